"""The shred path on the GPU: the device SHA-256, checks and Merkle roots
against hashlib and the Python reference, fdgpu_submit_shreds against the
oracle, the ring's slot semantics and the argument errors."""
import hashlib

import numpy as np
import pytest

import pyref_shred as ps
from firedancer_amd import VerifyEngine, workload
from firedancer_amd.ed25519 import CODE_SHRED_REJECT, SHRED_DTYPE, TXN_DTYPE

pytestmark = pytest.mark.gpu

VERSION = 0x1234
PRV = bytes(range(1, 33))


@pytest.fixture(scope="module")
def batch(oracle):
    return ps.verify_batch(VERSION, np.random.default_rng(21), workload.sign, oracle.verify)


@pytest.fixture(scope="module")
def matrix_batch():
    """the CPU tests' matrix and reject cases as one arena -> (arena, records, ok, roots)"""
    rng = np.random.default_rng(11)
    shreds = [b for b, _ in ps.matrix(PRV, VERSION, rng, workload.sign)]
    shreds += [bytearray(b) for b in ps.reject_cases(PRV, VERSION, np.random.default_rng(12), workload.sign).values()]
    arena, recs = ps.pack(shreds, [workload.sign(PRV, b"")[0]])
    roots = np.zeros((len(shreds), 32), dtype=np.uint8)
    ok = np.zeros(len(shreds), dtype=np.int8)
    for i, b in enumerate(shreds):
        r = ps.shred_root(b, VERSION)
        if r is None:
            ok[i] = CODE_SHRED_REJECT
        else:
            roots[i] = np.frombuffer(r, dtype=np.uint8)
    return arena, recs, ok, roots


def test_device_sha256_matches_hashlib(engine):
    rng = np.random.default_rng(9)
    blob = rng.integers(0, 256, 4096, dtype=np.uint8)
    lens = [0, 1, 55, 56, 63, 64, 65, 119, 120, 127, 128] + list(range(1100, 1261))
    recs = [(off, n, 0, 0, 1) for off in range(16) for n in lens]
    got = engine.debug_sha256(blob, np.array(recs, dtype=TXN_DTYPE))
    raw = blob.tobytes()
    for (off, n, *_), g in zip(recs, got):
        assert g.tobytes() == hashlib.sha256(raw[off:off + n]).digest(), (off, n)


def test_device_roots_match_python(engine, matrix_batch):
    arena, recs, want_ok, want_roots = matrix_batch
    assert len(recs) > 200 and (want_ok == 0).sum() > 200 and (want_ok != 0).sum() >= 18
    ok, roots = engine.debug_shred_roots(arena, recs, VERSION)
    assert ok.tolist() == want_ok.tolist()
    assert (roots == want_roots).all()


def test_verify_shreds_matches_the_oracle(engine, batch):
    arena, recs, want_codes, want_roots = batch
    codes, roots = engine.verify_shreds(arena, recs, VERSION)
    assert codes.tolist() == want_codes.tolist()
    assert (roots == want_roots).all()
    for kw in ({"key_cache": True}, {"full_path": True}):
        e = VerifyEngine(0, max_txn=1 << 10, max_sig=1 << 10, max_arena=1 << 20, **kw)
        try:
            c2, r2 = e.verify_shreds(arena, recs, VERSION)
        finally:
            e.close()
        assert c2.tolist() == want_codes.tolist(), kw
        assert (r2 == want_roots).all(), kw


def _take(batch, n, mode):
    """n records of the batch: mode 'mixed' as they come, 'reject' only shreds
    the checks drop, 'odd' a dropped shred in every odd lane and a passing one
    in every even lane."""
    arena, recs, codes, roots = batch
    good = np.flatnonzero(codes != CODE_SHRED_REJECT)
    bad = np.flatnonzero(codes == CODE_SHRED_REJECT)
    if mode == "mixed":
        idx = np.arange(n) % len(recs)
    elif mode == "reject":
        idx = bad[np.arange(n) % len(bad)]
    else:
        idx = np.where(np.arange(n) % 2 == 1, bad[np.arange(n) % len(bad)], good[np.arange(n) % len(good)])
    return arena, recs[idx], codes[idx], roots[idx]


@pytest.mark.parametrize("n,mode", [(0, "mixed"), (1, "mixed"), (63, "mixed"), (64, "mixed"), (65, "mixed"),
                                    (257, "mixed"), (1025, "mixed"), (257, "reject"), (1025, "odd")])
def test_batch_sizes(engine, batch, n, mode):
    arena, recs, want_codes, want_roots = _take(batch, n, mode)
    codes, roots = engine.verify_shreds(arena, recs, VERSION)
    assert len(codes) == n and roots.shape == (n, 32)
    assert codes.tolist() == want_codes.tolist()
    assert (roots == want_roots).all()
    if mode == "reject":
        assert (codes == CODE_SHRED_REJECT).all() and not roots.any()
    if mode == "odd":
        assert (codes[1::2] == CODE_SHRED_REJECT).all() and (codes[0::2] != CODE_SHRED_REJECT).all()


def test_two_batches_polled_in_reverse(engine, batch):
    arena, recs, want_codes, want_roots = batch
    reg = np.zeros(len(arena) + 8192, dtype=np.uint8)
    base = (-reg.ctypes.data) % 4096
    pinned = reg[base:base + len(arena)]
    pinned[:] = arena
    engine.host_register(pinned)
    try:
        half = len(recs) // 2
        t1 = engine.submit_shreds(pinned, recs[:half], VERSION)        # uploaded in place
        t2 = engine.submit_shreds(arena, recs[half:], VERSION)         # staged
        c2, r2 = engine.poll_shreds(t2)
        c1, r1 = engine.poll_shreds(t1)
    finally:
        engine.host_unregister(pinned)
    assert c1.tolist() == want_codes[:half].tolist() and c2.tolist() == want_codes[half:].tolist()
    assert (r1 == want_roots[:half]).all() and (r2 == want_roots[half:]).all()


def test_argument_errors(engine, batch):
    arena, recs, _, _ = batch

    def bad(r, a=arena):
        with pytest.raises(RuntimeError, match=r"\(-10\)"):            # FDGPU_ERR_INVAL
            engine.submit_shreds(a, r, VERSION)

    r = recs[:8].copy(); r["off"][3] = len(arena) - 100
    bad(r)
    r = recs[:8].copy(); r["pub_off"][0] = len(arena) - 31
    bad(r)
    big = np.zeros(4096, dtype=np.uint8)
    r = np.zeros(1, dtype=SHRED_DTYPE); r["sz"] = 1233
    bad(r, big)
    bad(np.zeros((1 << 17) + 1, dtype=SHRED_DTYPE))                    # n > max_txn
    # nothing was launched and no slot was taken: the ring still takes its two batches
    t1 = engine.submit_shreds(arena, recs[:4], VERSION)
    t2 = engine.submit_shreds(arena, recs[4:8], VERSION)
    engine.poll_shreds(t2); engine.poll_shreds(t1)
