"""Every shred of whole FEC sets to verdicts: one verify lane per set against
one per shred.

n full-size valid shreds (262,144 unless given) as n / 64 distinct 32:32 FEC
sets under one leader, shuffled, on one engine at ring_depth 2:
  (a) fdgpu_submit_shreds on these shreds (a verify lane per shred), two
      batches in flight: shreds/s
  (b) fdgpu_submit_shred_sets with no known roots (a lane per set): shreds/s
  (c) the same with the known root on all but each set's first shred
  (d) fdgpu_debug_shred_time and fdgpu_debug_shred_sets_time: the batch's
      ingest (for a set batch: ingest + dedup) against its verify, in ms of
      device time
Each rate is the median of --rounds rounds of --reps pipelined batches after a
warm-up batch.  One JSON line.
python tools/bench_shred_sets.py [--n 262144] [--rounds 5] [--reps 4]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import pyref_shred as ps  # noqa: E402
from firedancer_amd import VerifyEngine, _lib, workload  # noqa: E402
from firedancer_amd.ed25519 import SET_SHRED_DTYPE, SHRED_DTYPE, SHRED_NO_ROOT  # noqa: E402

VERSION = 0x1234


def make(n, seed=1):
    """n shreds of n / 64 distinct 32:32 sets, shuffled; the arena holds the
    shreds in set order, the leader key and every set's root
    -> (arena, set records without known roots, the same with them on all but
    each set's first shred in batch order)"""
    assert n % 64 == 0
    rng = np.random.default_rng(seed)
    prv = bytes(range(1, 33))
    blob, roots, sizes = [], [], []
    for k in range(n // 64):
        s, root = ps.fec_set(32, 32, ps.T_DATA, ps.T_CODE, prv, VERSION, rng, workload.sign, fec_set_idx=64 * k, slot=9 + k // 512)
        blob += [bytes(b) for b in s]
        sizes += [len(b) for b in s]
        roots.append(root)
    shreds_sz = sum(sizes)
    arena = np.frombuffer(b"".join(blob) + workload.sign(prv, b"")[0] + b"".join(roots), dtype=np.uint8).copy()
    recs = np.zeros(n, dtype=SET_SHRED_DTYPE)
    recs["sz"] = sizes
    recs["off"] = np.concatenate(([0], np.cumsum(sizes, dtype=np.uint64)[:-1]))
    recs["pub_off"] = shreds_sz
    recs["known_off"] = SHRED_NO_ROOT
    set_of = np.arange(n) // 64
    order = rng.permutation(n)
    recs, set_of = recs[order], set_of[order]
    known = recs.copy()
    first = np.zeros(n, dtype=bool)
    first[np.unique(set_of, return_index=True)[1]] = True
    known["known_off"] = np.where(first, SHRED_NO_ROOT, shreds_sz + 32 + 32 * set_of).astype(np.uint32)
    return arena, recs, known


def rate(submit, poll, n, rounds, reps):
    """median shreds/s over rounds, each reps batches with two in flight"""
    out = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        tk = [submit()]
        for _ in range(reps - 1):
            tk.append(submit())
            poll(tk.pop(0))
        poll(tk.pop(0))
        out.append(reps * n / (time.perf_counter() - t0))
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=4)
    a = ap.parse_args()
    info = _lib.require_product_build()
    n = a.n
    arena, recs, known = make(n)
    plain = np.zeros(n, dtype=SHRED_DTYPE)
    for k in ("off", "sz", "pub_off"):
        plain[k] = recs[k]
    eng = VerifyEngine(0, max_txn=n, max_sig=n, max_arena=len(arena) + 34 * n + 4096, ring_depth=2)
    try:
        c0, r0 = eng.verify_shreds(arena, plain, VERSION)                       # warm: buffers, workspace
        c1, r1, _, lanes1 = eng.verify_shred_sets(arena, recs, VERSION)
        c2, r2, _, lanes2 = eng.verify_shred_sets(arena, known, VERSION)
        assert (c0 == 0).all() and (c1 == 0).all() and (c2 == 0).all(), "a shred of the workload failed"
        assert (r0 == r1).all() and (r0 == r2).all()
        res = {"n": n, "sets": n // 64, "lanes_per_shred": n, "lanes_sets": lanes1, "lanes_sets_known": lanes2}
        for name, sub, pol in (("per_shred", lambda: eng.submit_shreds(arena, plain, VERSION), eng.poll_shreds),
                               ("sets", lambda: eng.submit_shred_sets(arena, recs, VERSION), eng.poll_shred_sets),
                               ("sets_known", lambda: eng.submit_shred_sets(arena, known, VERSION), eng.poll_shred_sets)):
            med, lo, hi = rate(sub, pol, n, a.rounds, a.reps)
            res[name + "_shreds_per_s"] = round(med)
            res[name + "_min_max"] = [round(lo), round(hi)]
        ing, vfy = eng.debug_shred_time(arena, plain, VERSION, iters=5)
        res["per_shred_ingest_ms"], res["per_shred_verify_ms"] = round(ing, 3), round(vfy, 3)
        ing, vfy = eng.debug_shred_sets_time(arena, recs, VERSION, iters=5)
        res["sets_ingest_dedup_ms"], res["sets_verify_ms"] = round(ing, 3), round(vfy, 3)
        ing, vfy = eng.debug_shred_sets_time(arena, known, VERSION, iters=5)
        res["sets_known_ingest_dedup_ms"], res["sets_known_verify_ms"] = round(ing, 3), round(vfy, 3)
    finally:
        eng.close()
    res.update(arena_mb=round(len(arena) / 1e6, 1), rounds=a.rounds, reps=a.reps,
               host_threads=min(16, os.cpu_count() or 1), build=info)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
