"""Raw shreds to verdicts: the fused GPU path against host-hashed roots.

For n full-size shreds under one leader key (n = 65,536 and 262,144 unless
given), on one engine at ring_depth 2:
  (a) fdgpu_submit_shreds / fdgpu_poll_shreds, two batches in flight: shreds/s
  (b) tile.shreds_verify over EngineVerifier (roots hashed on the host, up to
      16 threads, then the batched verify): shreds/s
  (c) fdgpu_debug_shred_time: the batch's ingest (checks + SHA-256 + records)
      against its verify, in ms of device time
One JSON line per n.  python tools/bench_shreds.py [--n 65536 262144] [--reps 6]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import pyref_shred as ps  # noqa: E402
from firedancer_amd import VerifyEngine, _lib, tile, workload  # noqa: E402

VERSION = 0x1234


def make(n, seed=1):
    """n shreds: whole 32+32 FEC sets of the three type pairs, repeated"""
    rng = np.random.default_rng(seed)
    prv = bytes(range(1, 33))
    base = []
    for td, tc in ((ps.T_DATA, ps.T_CODE), (ps.T_DATA_CH, ps.T_CODE_CH), (ps.T_DATA_RS, ps.T_CODE_RS), (ps.T_DATA, ps.T_CODE)):
        base += ps.fec_set(32, 32, td, tc, prv, VERSION, rng, workload.sign)[0]
    blob = b"".join(bytes(s) for s in base)
    sizes = np.array([len(s) for s in base], dtype=np.uint32)
    reps = (n + len(base) - 1) // len(base)
    arena = np.frombuffer(blob * reps + workload.sign(prv, b"")[0], dtype=np.uint8).copy()
    sz = np.tile(sizes, reps)[:n]
    recs = np.zeros(n, dtype=tile.SHRED_DTYPE)
    recs["sz"] = sz
    recs["off"] = np.concatenate(([0], np.cumsum(np.tile(sizes, reps), dtype=np.uint64)[:-1]))[:n]
    recs["pub_off"] = len(arena) - 32
    return arena, recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[65536, 262144])
    ap.add_argument("--reps", type=int, default=6)
    a = ap.parse_args()
    info = _lib.require_product_build()
    for n in a.n:
        arena, recs = make(n)
        eng = VerifyEngine(0, max_txn=n, max_sig=n, max_arena=len(arena) + 34 * n + 4096, ring_depth=2)
        try:
            codes, _ = eng.verify_shreds(arena, recs, VERSION)          # warm: buffers, workspace
            assert (codes == 0).all(), np.unique(codes, return_counts=True)
            t0 = time.perf_counter()
            tk = [eng.submit_shreds(arena, recs, VERSION)]
            for _ in range(a.reps - 1):
                tk.append(eng.submit_shreds(arena, recs, VERSION))
                eng.poll_shreds(tk.pop(0))
            eng.poll_shreds(tk.pop(0))
            fused = a.reps * n / (time.perf_counter() - t0)
            ver = tile.EngineVerifier([eng])
            c2, _ = tile.shreds_verify(ver, arena, recs, VERSION, batch_max=65536)
            assert (c2 == 0).all()
            t0 = time.perf_counter()
            for _ in range(max(1, a.reps // 2)):
                tile.shreds_verify(ver, arena, recs, VERSION, batch_max=65536)
            host = max(1, a.reps // 2) * n / (time.perf_counter() - t0)
            ver.close()
            ing, vfy = eng.debug_shred_time(arena, recs, VERSION, iters=5)
        finally:
            eng.close()
        print(json.dumps({"n": n, "fused_shreds_per_s": round(fused), "host_roots_shreds_per_s": round(host),
                          "ingest_ms": round(ing, 3), "verify_ms": round(vfy, 3), "host_threads": min(16, os.cpu_count() or 1),
                          "build": info}), flush=True)


if __name__ == "__main__":
    main()
