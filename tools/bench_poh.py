"""PoH chains on the GPU: bulk rate, a lone chain, the queue, and the host.

On one engine, the batch resident on the device (fdgpu_debug_poh_time: device
events around `iters` back-to-back runs after a warm-up run), `reps` times each:
  (a) hashes/s at a saturating batch: 131,072 tick entries of 4,096 hashes
  (b) the time of a single 62,500-hash chain alone
  (c) the time of 64 entries of 62,500 hashes together with 8,192 entries of
      64 hashes; with the queue working this is close to (b)
  (d) for scale, the host library's SHA-256 (fdt_sha256.h) iterated on 32-byte
      inputs over 16 host threads (fdgpu_poh_verify_host), on the same box
One JSON line.  python tools/bench_poh.py [--reps 3] [--iters 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from firedancer_amd import VerifyEngine, _lib, tile  # noqa: E402
from firedancer_amd.ed25519 import POH_DTYPE, POH_NO_MIX  # noqa: E402


def ticks(counts, seed=1):
    """tick entries of the given hash counts from random start hashes (the claimed hash is the start hash: every
    entry is computed in full and reported as a mismatch, which costs what a match costs)"""
    n = len(counts)
    arena = np.random.default_rng(seed).integers(0, 256, 32 * n, dtype=np.uint8)
    en = np.zeros(n, dtype=POH_DTYPE)
    en["hash_cnt"] = counts
    en["prev_off"] = en["hash_off"] = 32 * np.arange(n)
    en["mix_off"] = POH_NO_MIX
    return arena, en, np.zeros(0, dtype=np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    info = _lib.require_product_build()
    cap = 1 << 16
    cases = {"a": [4096] * 131072, "b": [62500], "c": [62500] * 64 + [64] * 8192}
    out = {}
    eng = VerifyEngine(0, max_txn=1 << 17, max_sig=1 << 10, max_arena=1 << 23)
    try:
        for name, counts in cases.items():
            batch = ticks(counts)
            codes, _ = eng.debug_poh(*batch, cap)                       # warm: code objects, the clocks
            assert len(codes) == len(counts)
            ms = [eng.debug_poh_time(*batch, cap, iters=a.iters if name == "a" else max(1, a.iters // 2))[1]
                  for _ in range(a.reps)]
            out[name + "_chain_ms"] = [round(x, 3) for x in ms]
            if name == "a":
                out["a_hashes_per_s"] = [round(sum(counts) / (x * 1e-3)) for x in ms]
        out["b_us_per_hash"] = [round(x * 1e3 / 62500, 3) for x in out["b_chain_ms"]]
        out["c_over_b"] = round(min(out["c_chain_ms"]) / min(out["b_chain_ms"]), 3)
    finally:
        eng.close()
    threads = min(16, os.cpu_count() or 1)
    batch = ticks([250000] * (4 * threads))
    tile.poh_verify_host(*ticks([1000] * threads), cap << 4)
    host = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        tile.poh_verify_host(*batch, 1 << 20)
        host.append(round(250000 * 4 * threads / (time.perf_counter() - t0)))
    out.update({"d_host_hashes_per_s": host, "host_threads": threads, "iters": a.iters, "build": info})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
