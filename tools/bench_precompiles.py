#!/usr/bin/env python3
"""Ed25519 precompile instructions: the fused ring batch (fdgpu_submit_precompiles /
fdgpu_poll_precompiles: parse, walk and verify on the GPU) against the host-walk baseline
(fdgpu_precompiles_verify over the engine verifier: parse and walk on up to 16 host threads, the
records verified in batches on the same engine), and the device time of the ingest and the verify
alone (fdgpu_debug_precompile_time).

    python tools/bench_precompiles.py [--txns 4096,32768] [--reps 5] [--out FILE]

Shapes: every transaction carries one Ed25519 instruction with 1 or 8 records: one record over a
message of 100 or 900 bytes, or 8 records (their signatures and keys take 768 bytes of the 1,232)
over 12-byte messages.  Prints one
JSON line per (batch size, shape).  Not measured here: grouping a wave's signatures by SHA-512
block count (the verify's block loop runs to the wave's longest message), which the ring batch
leaves out.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

import pyref_precompile as pp                              # noqa: E402  (the transaction builder)
from firedancer_amd import VerifyEngine, _lib, tile, workload   # noqa: E402
from firedancer_amd import ed25519 as ed                   # noqa: E402

SHAPES = {"1x100": [100], "1x900": [900], "8x12": [12] * 8}


def make(n, lens, distinct=64):
    g = pp.Gen(workload.sign, "bench %r" % (lens,))
    accts = [g.payer, pp.ED25519_ID]
    base = [g.case("b", [(1, b"", g.self_ix(lens))], accts=accts).payload for _ in range(distinct)]
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    info = _lib.require_product_build()
    sizes = [int(x) for x in a.txns.split(",")]
    eng = VerifyEngine(0, max_txn=max(sizes), max_sig=8 * max(sizes), max_arena=1300 * max(sizes))
    ver = tile.EngineVerifier([eng])
    lines = []
    try:
        for n in sizes:
            for name, lens in SHAPES.items():
                payloads = make(n, lens)
                arena = np.frombuffer(b"".join(payloads), dtype=np.uint8)
                recs = np.zeros(n, dtype=ed.PRECOMPILE_DTYPE)
                recs["sz"] = [len(p) for p in payloads]
                recs["off"][1:] = np.cumsum(recs["sz"][:-1])
                recs["sig_cap"] = len(lens)
                # the baseline's batches: half of the records each (two in flight), within the engine's limits --
                # a record is one single-signature transaction of the verifier
                bm = min((n * len(lens) + 1) // 2, max(sizes))
                codes, _ = eng.verify_precompiles(arena, recs)
                hc, _ = tile.precompiles_verify(ver, payloads, batch_max=bm)
                assert not codes.any() and not hc.any()
                fused = median_ms(lambda: eng.verify_precompiles(arena, recs), a.reps)
                host = median_ms(lambda: tile.precompiles_verify(ver, payloads, batch_max=bm), a.reps)
                ing, vfy = eng.debug_precompile_time(arena, recs, iters=a.reps)
                line = {"txns": n, "shape": name, "sigs": n * len(lens), "fused_ms_median_min_max": fused,
                        "host_walk_ms_median_min_max": host, "host_batch_max": bm, "ingest_ms": ing, "verify_ms": vfy,
                        "ingest_share_of_verify": ing / vfy, "reps": a.reps, "build": info}
                print(json.dumps(line), flush=True)
                lines.append(line)
    finally:
        ver.close()
        eng.close()
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
