#!/usr/bin/env python3
"""secp256k1 precompile instructions: the fused ring batch (fdgpu_submit_secp256k1 /
fdgpu_poll_secp256k1: parse, walk and every record's Keccak + recover + Keccak on the GPU)
against the host path (fdgpu_secp256k1_verify_host: the same source compiled by g++, on up to 16
threads) over the same bytes, and the device time of the ingest and of the recover kernel alone
(fdgpu_debug_secp256k1_time).

    python tools/bench_secp256k1.py [--txns 4096,32768] [--reps 3] [--out FILE]

Shapes: every transaction carries one secp256k1 instruction with one record, over a message of
100 bytes, or ("mixed") over messages of 0..998 bytes that change from one transaction to the
next, so that every wave of the recover kernel holds the whole range and its block loop runs to
the longest.  Prints one JSON line per (batch size, shape).  The baseline is the host path, never
the code under test against itself.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

import pyref_secp256k1 as k1                               # noqa: E402  (the transaction builder)
from firedancer_amd import VerifyEngine, _lib, tile        # noqa: E402
from firedancer_amd import ed25519 as ed                   # noqa: E402

MIXED = [0, 998, 1, 135, 136, 137, 271, 272, 500, 64, 700, 32, 900, 408, 10, 998]


def make(n, shape, distinct=64):
    g = k1.Gen("bench " + shape)
    accts = [g.payer, k1.SECP256K1_ID]
    base = []
    for i in range(distinct):
        ln = 100 if shape == "1x100" else MIXED[i % len(MIXED)]
        # a long message does not fit beside its signature: there the signature lies inside it (Gen.long_ix)
        data = g.long_ix(ln) if ln > 900 else g.self_ix([ln])
        base.append(g.case("b", [(1, b"", data)], accts=accts).payload)
    return [base[i % distinct] for i in range(n)]


def median_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--txns", default="4096,32768")
    ap.add_argument("--shapes", default="1x100,mixed")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    info = _lib.require_product_build()
    sizes = [int(x) for x in a.txns.split(",")]
    eng = VerifyEngine(0, max_txn=max(sizes), max_sig=max(sizes), max_arena=1300 * max(sizes))
    lines = []
    try:
        for n in sizes:
            for shape in a.shapes.split(","):
                if shape == "mixed" and n != sizes[0]:
                    continue                                   # one batch of mixed lengths
                payloads = make(n, shape)
                arena = np.frombuffer(b"".join(payloads), dtype=np.uint8)
                recs = np.zeros(n, dtype=ed.PRECOMPILE_DTYPE)
                recs["sz"] = [len(p) for p in payloads]
                recs["off"][1:] = np.cumsum(recs["sz"][:-1])
                recs["sig_cap"] = 1
                codes, _ = eng.verify_secp256k1(arena, recs)
                hc, _ = tile.secp256k1_verify_host(payloads)
                assert not codes.any() and not hc.any()
                fused = median_ms(lambda: eng.verify_secp256k1(arena, recs), a.reps)
                host = median_ms(lambda: tile.secp256k1_verify_host(payloads), a.reps)
                ing, rec = eng.debug_secp256k1_time(arena, recs, iters=a.reps)
                line = {"txns": n, "shape": shape, "records": n, "fused_ms_median_min_max": fused,
                        "host_16_threads_ms_median_min_max": host, "host_threads": min(16, os.cpu_count() or 1),
                        "fused_speedup_over_host": host[0] / fused[0], "ingest_ms": ing, "recover_ms": rec,
                        "recover_records_per_s": n / (rec * 1e-3), "reps": a.reps, "build": info}
                print(json.dumps(line), flush=True)
                lines.append(line)
    finally:
        eng.close()
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
