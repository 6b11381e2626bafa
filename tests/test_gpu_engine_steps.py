"""The host engine's shared steps (csrc/fdgpu_engine.h): shred, PoH and frag
batches alternating through one ring slot and its one result pair, empty
batches between full ones, the staged split upload of shred and PoH arenas
against the same batch from a registered buffer, and the stage-timing
diagnostics.  Codes and 32-byte items are compared with the oracle and the
hashlib models, bit for bit."""
import ctypes
import math

import numpy as np
import pytest

import pyref_poh as pp
import pyref_shred as ps
from firedancer_amd import VerifyEngine, _lib, tile, workload
from firedancer_amd.ed25519 import CODE_PARSE_FAIL, FRAG_DTYPE, FRAG_EX_DTYPE, FragBatch

pytestmark = pytest.mark.gpu

VERSION = 0x1234
CAP = 1 << 16
SPLIT_MIN = 4 << 20             # FDGPU_COPY_SPLIT_MIN: arenas from here on are staged in four parts
SIZES = (1, 64, 65)             # either side of the results' 64-byte code padding


@pytest.fixture(scope="module")
def one_slot():
    """ring_depth = 1: every batch goes through the same slot; the arena admits the padded ones"""
    e = VerifyEngine(0, max_txn=1 << 10, max_sig=1 << 11, max_arena=5 << 20, ring_depth=1)
    yield e
    e.close()


@pytest.fixture(scope="module")
def shreds(oracle):
    """-> (arena, records, codes, roots): about 400 shreds, shuffled so that every run of 65 holds accepted, dropped
    and badly signed ones"""
    arena, recs, codes, roots = ps.verify_batch(VERSION, np.random.default_rng(21), workload.sign, oracle.verify)
    order = np.random.default_rng(22).permutation(len(recs))
    recs, codes, roots = recs[order], codes[order], roots[order]
    for lo in (0, 65, 100, 200):
        assert len(set(codes[lo:lo + 64].tolist())) >= 3, lo
    return arena, recs, codes, roots


@pytest.fixture(scope="module")
def poh():
    """-> (arena, entries, sig_offs, (codes, hashes)): 200 entries, a few of them spoiled"""
    rng = np.random.default_rng(57)
    arena, entries, sig_offs = pp.mixed(200, rng, lo=1, hi=300).arrays()
    for i, how in ((0, "hash"), (63, "prev"), (64, "cnt+"), (66, "hash"), (129, "prev")):
        pp.corrupt(arena, entries, sig_offs, i, how, rng)
    want = pp.evaluate(arena, entries, sig_offs, CAP)
    assert 0 < np.count_nonzero(want[0][:65]) < 65
    return arena, entries, sig_offs, want


@pytest.fixture(scope="module")
def frags(oracle):
    """-> (arena, frag records with their trailers' places, codes, the parsed txn per frag or None): 65 payloads, two
    of them garbage"""
    a, t, _ = workload.cfg1(65, seed=0x57E9)
    payloads = workload.payloads(a, t)
    payloads[7], payloads[64] = b"\x00" * 40, payloads[64][:50]
    offs = np.cumsum([0] + [(len(p) + 15) // 16 * 16 for p in payloads])
    arena = np.zeros(int(offs[-1]) + 256, dtype=np.uint8)
    fx = np.zeros(len(payloads), dtype=FRAG_EX_DTYPE)
    td = np.zeros(len(payloads), dtype=workload.TXN_DTYPE)
    raws, tr = [], 0
    for k, p in enumerate(payloads):
        o = int(offs[k])
        arena[o:o + len(p)] = np.frombuffer(p, dtype=np.uint8)
        fp, raw = tile.txn_parse(p)
        fx[k] = (o, len(p), tr, fp)
        tr += (fp + 3) & ~3
        raws.append(raw if fp else None)
        if fp:
            d = tile.txn_decode(raw)
            td[k] = (o + d["message_off"], len(p) - d["message_off"], o + d["signature_off"], o + d["acct_addr_off"],
                     d["signature_cnt"])
    codes = oracle.verify_txns(arena, td)
    codes[[7, 64]] = CODE_PARSE_FAIL
    return arena, fx, codes, raws


def check_shreds(got, shreds, lo, n):
    _, _, want_codes, want_roots = shreds
    codes, roots = got
    assert codes.tolist() == want_codes[lo:lo + n].tolist()
    assert roots.shape == (n, 32) and (roots == want_roots[lo:lo + n]).all()


def check_poh(got, poh, lo, n):
    want_codes, want_hashes = poh[3]
    codes, hashes = got
    assert codes.tolist() == want_codes[lo:lo + n].tolist()
    assert hashes.shape == (n, 32) and (hashes == want_hashes[lo:lo + n]).all()


def run_frags(e, frags, n):
    arena, fx, want, raws = frags
    fx = fx[:n]
    tr_sz = int(fx["tr_off"][-1]) + ((int(fx["tr_cap"][-1]) + 3) & ~3) if n else 0
    codes, trailers = e.poll_frags(e.submit_frags(arena, fx, tr_sz))
    assert codes.tolist() == want[:n].tolist()
    for k in range(n):
        if raws[k] is not None:
            o = int(fx["tr_off"][k])
            assert bytes(trailers[o:o + len(raws[k])]) == raws[k], k


@pytest.mark.parametrize("n", SIZES)
def test_kinds_alternate_through_one_slot(one_slot, shreds, poh, frags, n):
    """shreds -> PoH -> other shreds -> frags -> other PoH entries, all in the one slot: each batch's read-back is its
    own, whatever kind and size the slot carried before"""
    e = one_slot
    sh_arena, recs = shreds[:2]
    p_arena, entries, sig_offs = poh[:3]
    check_shreds(e.verify_shreds(sh_arena, recs[:n], VERSION), shreds, 0, n)
    check_poh(e.verify_poh(p_arena, entries[:n], sig_offs, CAP), poh, 0, n)
    check_shreds(e.verify_shreds(sh_arena, recs[100:100 + n], VERSION), shreds, 100, n)
    run_frags(e, frags, n)
    check_poh(e.verify_poh(p_arena, entries[65:65 + n], sig_offs, CAP), poh, 65, n)


def test_empty_batches_between_full_ones(one_slot, shreds, poh, frags):
    e = one_slot
    sh_arena, recs = shreds[:2]
    p_arena, entries, sig_offs = poh[:3]
    check_shreds(e.verify_shreds(sh_arena, recs[:65], VERSION), shreds, 0, 65)
    check_shreds(e.verify_shreds(sh_arena, recs[:0], VERSION), shreds, 0, 0)
    check_shreds(e.verify_shreds(sh_arena, recs[200:265], VERSION), shreds, 200, 65)
    check_poh(e.verify_poh(p_arena, entries[:65], sig_offs, CAP), poh, 0, 65)
    check_poh(e.verify_poh(p_arena, entries[:0], sig_offs[:0], CAP), poh, 0, 0)
    check_poh(e.verify_poh(p_arena, entries[100:165], sig_offs, CAP), poh, 100, 65)
    run_frags(e, frags, 65)
    run_frags(e, frags, 0)
    run_frags(e, frags, 64)
    check_shreds(e.verify_shreds(sh_arena, recs[:0], VERSION), shreds, 0, 0)
    check_poh(e.verify_poh(p_arena, entries[:64], sig_offs, CAP), poh, 0, 64)


def at_the_end(arena, sz):
    """the arena's bytes as the last ones of a zeroed arena of sz bytes, i.e. in the staging's ragged last part
    -> (padded arena, the offset its bytes moved by)"""
    part = ((sz + 3) // 4 + 63) & ~63                 # stage_arena's part of four (FDGPU_COPY_THREADS)
    base = sz - len(arena)
    assert sz >= SPLIT_MIN and base >= 3 * part and (sz - 3 * part) % 64
    out = np.zeros(sz, dtype=np.uint8)
    out[base:] = arena
    return out, base


def registered(e, arena):
    """a page-aligned copy of arena, registered with the engine -> (the copy, its backing buffer)"""
    back = np.zeros(len(arena) + 8192, dtype=np.uint8)
    o = (-back.ctypes.data) % 4096
    pinned = back[o:o + len(arena)]
    pinned[:] = arena
    e.host_register(pinned)
    return pinned, back


@pytest.mark.parametrize("sz", [SPLIT_MIN + 1, SPLIT_MIN + 64 * 4 + 1])
def test_split_upload_of_shreds_and_poh(one_slot, shreds, poh, sz):
    """an unregistered arena just over the split threshold is staged in four parts, the last one ragged and holding
    the whole batch; the same bytes from a registered buffer are uploaded in place"""
    e = one_slot
    sh_arena, recs = shreds[:2]
    big, base = at_the_end(sh_arena, sz)
    recs = recs[:65].copy()
    recs["off"] += base
    recs["pub_off"] += base
    check_shreds(e.verify_shreds(big, recs, VERSION), shreds, 0, 65)
    pinned, _back = registered(e, big)
    try:
        check_shreds(e.verify_shreds(pinned, recs, VERSION), shreds, 0, 65)
    finally:
        e.host_unregister(pinned)

    p_arena, entries, sig_offs = poh[:3]
    big, base = at_the_end(p_arena, sz)
    entries = entries[:65].copy()
    for f in ("prev_off", "hash_off"):
        entries[f] += base
    entries["mix_off"][entries["mix_off"] != pp.POH_NO_MIX] += base
    sig_offs = sig_offs + np.uint32(base)
    check_poh(e.verify_poh(big, entries, sig_offs, CAP), poh, 0, 65)
    pinned, _back = registered(e, big)
    try:
        check_poh(e.verify_poh(pinned, entries, sig_offs, CAP), poh, 0, 65)
    finally:
        e.host_unregister(pinned)


def test_stage_timers(one_slot, shreds, poh):
    """fdgpu_debug_shred_time and fdgpu_debug_poh_time: two finite, non-negative means; a ring batch on the same
    engine straight afterwards is right; iters = 0 and a null out-pointer are argument errors"""
    e, L = one_slot, _lib.lib()
    sh_arena, recs = shreds[:2]
    p_arena, entries, sig_offs = poh[:3]
    for t in e.debug_shred_time(sh_arena, recs[:65], VERSION, iters=2):
        assert math.isfinite(t) and t >= 0
    check_shreds(e.verify_shreds(sh_arena, recs[:65], VERSION), shreds, 0, 65)
    for t in e.debug_poh_time(p_arena, entries[:65], sig_offs, CAP, iters=2):
        assert math.isfinite(t) and t >= 0
    check_poh(e.verify_poh(p_arena, entries[:65], sig_offs, CAP), poh, 0, 65)
    with pytest.raises(RuntimeError, match=r"\(-10\)"):               # FDGPU_ERR_INVAL
        e.debug_shred_time(sh_arena, recs[:65], VERSION, iters=0)
    with pytest.raises(RuntimeError, match=r"\(-10\)"):
        e.debug_poh_time(p_arena, entries[:65], sig_offs, CAP, iters=0)
    r, en, so = np.ascontiguousarray(recs[:65]), np.ascontiguousarray(entries[:65]), np.ascontiguousarray(sig_offs)
    ms = ctypes.c_double()
    for outs in ((None, ctypes.byref(ms)), (ctypes.byref(ms), None)):
        assert L.fdgpu_debug_shred_time(e._h, sh_arena.ctypes.data, sh_arena.size, r.ctypes.data, 65, VERSION, 2, *outs) == -10
        assert L.fdgpu_debug_poh_time(e._h, p_arena.ctypes.data, p_arena.size, en.ctypes.data, 65, so.ctypes.data, len(so),
                                      CAP, 2, *outs) == -10
    check_shreds(e.verify_shreds(sh_arena, recs[65:130], VERSION), shreds, 65, 65)


def test_dev_batch_time2(one_slot, oracle):
    """fdgpu_dev_batch_time2 on a signature batch and on a frag batch: finite, non-negative times, and the batch still
    verifies to the oracle's codes"""
    e = one_slot
    arena, txns, _ = workload.cfg1(65, seed=0x71E2)
    want = oracle.verify_txns(arena, txns)
    fr = np.zeros(len(txns), dtype=FRAG_DTYPE)
    fr["off"] = txns["sig_off"] - 1
    fr["sz"] = txns["msg_off"] + txns["msg_sz"] - fr["off"]
    for b in (e.upload(arena, txns), e.upload_frags(arena, fr)):
        try:
            for t in FragBatch.time2(b, 2):
                assert math.isfinite(t) and t >= 0
            b.verify()
            assert b.codes().tolist() == want.tolist()
        finally:
            b.free()
