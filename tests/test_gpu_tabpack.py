"""The packed table entry of the verify chain (csrc/fdgpu_atab.h): a cached
point's four coordinates in 8 words each, one 128-B line an entry.

* fdgpu_debug_tabpack runs atab_store, atab_load and the LDS path
  (stage_entry + unstage_entry_signed, both signs) on given limbs: every
  residue must come back, within the R bound, Y+X / Y-X swapped for neg, and
  the stored 32 words must equal the same packing done here in numpy.
* The verify itself at the smallest sizes at which the layout can go wrong
  (a partial wave, a partial block, the workspace's last lane): the one-lane
  kernel, the pair kernel, the key cache with a pool of 1 and of n, the
  full-length fallback (it reads -R entry 1 and the parked [S]B) and the
  spread launch, each against the oracle's codes.
"""
import re
import subprocess

import numpy as np
import pytest

import firedancer_amd as fa
from firedancer_amd import _lib, workload

from test_gpu_parity import _vector_batch

P = 2**255 - 19
WIDTH = [26, 25] * 5
SHIFT = [0, 26, 51, 77, 102, 128, 153, 179, 204, 230]
TIGHT = np.array([(1 << w) - 1 for w in WIDTH], dtype=np.uint64)
# the R bound of csrc/fdgpu_fe.h: limbs <= 2^26, + 2^17.2 on limbs 1 and 5
R_MAX = np.array([(1 << 26) + (150562 if i in (1, 5) else 0) for i in range(10)], dtype=np.uint64)


def limbs_of(x):
    return [(x >> SHIFT[i]) & ((1 << WIDTH[i]) - 1) for i in range(10)]


def value_of(limbs):
    return sum(int(l) << SHIFT[i] for i, l in enumerate(limbs))


def coordinates():
    """The issue's inputs, as rows of 10 limbs."""
    rng = np.random.default_rng(0x7AB)
    rows = [[0] * 10, limbs_of(P - 1), [int(t) for t in TIGHT], [int(r) for r in R_MAX]]
    one = [int(rng.integers(0, int(t) + 1)) for t in TIGHT]
    one[1] = 1 << 25                                         # what fe_carry can leave
    rows.append(one)
    rows += [limbs_of(v) for v in range(P, 2**255)]          # non-canonical values, tight limbs
    rows += [[int(rng.integers(0, int(t) + 1)) for t in TIGHT] for _ in range(100)]
    rows += [[int(rng.integers(0, int(r) + 1)) for r in R_MAX] for _ in range(100)]
    return np.array(rows, dtype=np.uint64)


def host_tight(c):
    """fe_tight: two linear carries, limb 9's excess into limb 0 times 19."""
    c = c.astype(np.uint64).copy()
    for _ in range(2):
        for i in range(9):
            c[:, i + 1] += c[:, i] >> np.uint64(WIDTH[i])
            c[:, i] &= TIGHT[i]
        top = c[:, 9] >> np.uint64(25)
        c[:, 9] &= TIGHT[9]
        c[:, 0] += np.uint64(19) * top
    return c


def host_pack(c):
    """Tight limbs [n, 10] -> packed words [n, 8]: limb 8 over the spare high
    bits of words 0..3 (6, 7, 6, 7), limb 9 over those of words 4..7."""
    w = np.zeros((len(c), 8), dtype=np.uint64)
    for h in range(2):
        s = c[:, 8 + h]
        for k, (lo, wd) in enumerate(((0, 26), (6, 25), (13, 26), (19, 25))):
            w[:, 4 * h + k] = c[:, 4 * h + k] | (((s >> np.uint64(lo)) << np.uint64(wd)) & np.uint64(0xFFFFFFFF))
    return w.astype(np.uint32)


def stored_pos(c, j):
    return 8 * c + j if c >= 2 else 4 * (j // 2) + 2 * c + j % 2


def test_tabpack_diagnostic_is_internal():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "fdgpu_debug_tabpack" in set(re.findall(r"\s[TW]\s(\w+)$", out, flags=re.M))
    assert "fdgpu_debug_tabpack" not in _lib.header_functions()


def test_host_packing_round_trips():
    """The numpy packing the GPU's is compared with keeps every residue."""
    co = coordinates()
    t = host_tight(co)
    assert (t <= TIGHT).all()
    for a, b in zip(co, t):
        assert value_of(a) % P == value_of(b) % P
    w = host_pack(t).astype(np.uint64)
    for j in range(8):
        assert ((w[:, j] & TIGHT[j]) == t[:, j]).all()


@pytest.mark.gpu
def test_tabpack_round_trip(engine):
    co = coordinates()
    m, n = len(co), 256                                       # four waves; every input in every coordinate slot
    assert m <= n
    idx = (np.arange(n)[:, None] + 61 * np.arange(4)[None, :]) % m
    ent = co[idx]                                             # [n, 4, 10]
    stored, back = engine.debug_tabpack(ent.reshape(n, 40).astype(np.uint32))
    # the stored line, bit for bit
    exp = np.zeros((n, 32), dtype=np.uint32)
    for c in range(4):
        w = host_pack(host_tight(ent[:, c]))
        for j in range(8):
            exp[:, stored_pos(c, j)] = w[:, j]
    assert (stored == exp).all(), np.argwhere(stored != exp)[:10]
    back = back.reshape(n, 3, 4, 10).astype(np.uint64)
    assert (back <= R_MAX).all() and (back <= TIGHT).all()
    load, pos, neg = back[:, 0], back[:, 1], back[:, 2]
    assert (load == pos).all()
    assert (neg[:, 0] == pos[:, 1]).all() and (neg[:, 1] == pos[:, 0]).all() and (neg[:, 2:] == pos[:, 2:]).all()
    for i in range(n):
        for c in range(4):
            assert value_of(load[i, c]) % P == value_of(ent[i, c]) % P, (i, c)


SIZES = [1, 63, 64, 65, 255, 256, 257]
CONFIGS = {"one": {}, "pair": {"pair": True}, "kcache": {"key_cache": True}, "kfull": {"full_path": True},
           "kfull_kcache": {"full_path": True, "key_cache": True}, "spread": {"spread": True},
           "spread_pair": {"spread": True, "pair": True}}


@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(name):
        if name not in made:
            made[name] = fa.VerifyEngine(0, max_txn=8192, **CONFIGS[name])
        return made[name]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def batches(oracle):
    """(n, key_pool) -> (arena, txns, the oracle's codes), computed once."""
    made = {}

    def get(n, pool=0):
        if (n, pool) not in made:
            arena, txns, _ = workload.make_txns(n, 0x7AB0 + n, corrupt=0.10, key_pool=pool)
            made[(n, pool)] = (arena, txns, oracle.verify_txns(arena, txns, nthreads=8))
        return made[(n, pool)]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_small_batches_match_oracle(engines, batches, cfg, n):
    pools = (1, n) if "kcache" in cfg else (0,)
    for pool in pools:
        arena, txns, exp = batches(n, pool)
        got = engines(cfg).verify_txns(arena, txns)
        assert (got == exp).all(), (cfg, n, pool, np.nonzero(got != exp)[0][:10])


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_golden_vectors_every_path(engines, vectors, cfg):
    vs, arena, txns = _vector_batch(vectors)
    codes = engines(cfg).verify_txns(arena, txns)
    bad = [(v["src"], v["tc_id"], v["code"], int(c)) for v, c in zip(vs, codes) if c != v["code"]]
    assert not bad, (cfg, bad[:20])
