"""The verify chain at chosen k, through the prehashed kernels.

A hash gives uniformly random k: the rest of the suite only ever runs waves of
31..34 windows and a fallback queue that is empty or (forced) holds every
lane.  fdgpu_debug_verify_prehashed hands verify_hs_body<false, true> and
fdgpu_verify_pair_kernel<true> -- the product's body source, reading k's
SHA-512 state instead of hashing -- the records of tests/pyref_chain.py, lane
i = descriptor i, so each launch below is a chosen arrangement of window
counts and of lanes that take the full-length path.  Every code must equal the
exact verdict ([S]B == R + [k]A evaluated in Python integers), and the
fallback queue's final count the model's number of full routes among the lanes
that passed pass 1; under FDGPU_FLAG_KFULL the codes stay and the count is
every such lane.
"""
import re
import subprocess

import numpy as np
import pytest

from firedancer_amd import _lib
from firedancer_amd.ed25519 import SIG_DESC_DTYPE

import pyref_chain as pc


def test_chain_diagnostic_is_internal():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "fdgpu_debug_verify_prehashed" in set(re.findall(r"\s[TW]\s(\w+)$", out, flags=re.M))
    assert "fdgpu_debug_verify_prehashed" not in _lib.header_functions()


@pytest.fixture(scope="module")
def chain():
    """The record set, its arena, and the named lane orders (lists of record indices), built once."""
    rs = pc.RecordSet()
    arena, offs = rs.arena()
    n_rec = len(rs.records)
    plain = [i for i in range(n_rec) if rs.records[i].tors is None]
    half = [i for i in plain if rs.route_of(i).kind == "half"]
    full = rs.full()
    assert half and len(full) >= 30

    def cyc(src, n, start=0):
        return [src[(start + j) % len(src)] for j in range(n)]

    orders = {}
    # (a) a wave whose 64 lanes all run the same number of windows
    for c in (1, 2, 3, 32, 33, 34, 39, 40):
        orders[f"wave_all_{c}"] = cyc(rs.half_at(c), 64)
    # (b) one wave mixing every count 1..40: the wave's maximum is 40, the one-window lanes lead with 39 zeros
    one_each = [rs.half_at(c)[c % len(rs.half_at(c))] for c in range(1, 41)]
    orders["wave_mixed_1_40"] = one_each + [rs.half_at(c)[(c + 1) % len(rs.half_at(c))] for c in range(1, 25)]
    # two waves: counts 1..3 only beside counts 38..40 only
    orders["waves_short_long"] = cyc(rs.half_at(1) + rs.half_at(2) + rs.half_at(3), 64) + \
        cyc(rs.half_at(38) + rs.half_at(39) + rs.half_at(40), 64)
    # (c) a partial wave and a partial block, over everything (half and full lanes as they come)
    for n in (1, 63, 65, 257):
        orders[f"partial_{n}"] = cyc(plain, n, start=7 * n)
    # (d) full lanes among half-size ones
    orders["full_lane0"] = [full[0]] + cyc(half, 63, 11)
    orders["full_lane63"] = cyc(half, 63, 29) + [full[1]]
    orders["full_alternating"] = [x for j in range(32) for x in (full[j % len(full)], half[(5 * j) % len(half)])]
    orders["full_all64"] = cyc(full, 64)
    orders["full_between_halves"] = [half[3], full[2], half[4]]
    orders["carry_lane_among_halves"] = cyc(rs.half_at(33), 20) + rs.by_k[rs.classes[("carry",)]] + cyc(rs.half_at(40), 9)
    # u = 0: the A lane's chain is all zeros (k = 0; its S = 0 record has R = O and fails pass 1)
    orders["u_zero"] = rs.by_k[0] + cyc(rs.half_at(2), 3) + rs.by_k[0] + rs.by_k[1]
    # (e) more full lanes than the fallback's one block has threads, in three blocks of lanes
    orders["full_over_256"] = [full[j % len(full)] if j % 2 == 0 or j >= 300 else half[j % len(half)] for j in range(700)]
    # every record once, and the torsion set
    orders["all_records"] = list(range(n_rec))
    orders["torsion"] = [i for res in range(8) for i in rs.tors[res]]
    assert rs.n_full(orders["full_over_256"]) > 256
    assert rs.n_full(orders["wave_mixed_1_40"]) == 0 and rs.n_full(orders["full_lane0"]) == 1
    return rs, arena, offs, orders


ORDERS = [f"wave_all_{c}" for c in (1, 2, 3, 32, 33, 34, 39, 40)] + [
    "wave_mixed_1_40", "waves_short_long", "partial_1", "partial_63", "partial_65", "partial_257", "full_lane0",
    "full_lane63", "full_alternating", "full_all64", "full_between_halves", "carry_lane_among_halves", "u_zero",
    "full_over_256", "all_records", "torsion"]


def _run(engine, chain, name, pair, forced):
    rs, arena, offs, orders = chain
    idx = orders[name]
    exp = rs.expected[idx]
    codes, n_full = engine.debug_verify_prehashed(arena, rs.descs(idx, offs, SIG_DESC_DTYPE), full=forced, pair=pair)
    bad = [(lane, i, rs.records[i].kind, hex(rs.records[i].k), rs.route_of(i).kind, rs.route_of(i).nd, int(codes[lane]),
            int(exp[lane])) for lane, i in enumerate(idx) if codes[lane] != exp[lane]]
    print(f"{name} pair={pair} forced={forced}: n={len(idx)} n_full={n_full} model={rs.n_full(idx)} "
          f"pass1={rs.n_pass1(idx)} wrong={len(bad)}")
    assert not bad, (name, pair, forced, len(bad), bad[:8])
    assert n_full == (rs.n_pass1(idx) if forced else rs.n_full(idx)), (name, pair, forced)


def test_orders_are_all_run(chain):
    assert sorted(ORDERS) == sorted(chain[3])


@pytest.mark.gpu
@pytest.mark.parametrize("pair", [False, True], ids=["one", "pair"])
@pytest.mark.parametrize("name", ORDERS)
def test_chain_codes_and_queue_count(engine, chain, name, pair):
    _run(engine, chain, name, pair, False)


@pytest.mark.gpu
@pytest.mark.parametrize("pair", [False, True], ids=["one", "pair"])
@pytest.mark.parametrize("name", ORDERS)
def test_chain_forced_full_same_codes(engine, chain, name, pair):
    _run(engine, chain, name, pair, True)


@pytest.mark.gpu
def test_torsion_verdict_at_every_k_mod_8(engine, chain):
    """A + T for the eight torsion points, S and S + 1, at a k of every residue mod 8: the kernel's u is v k mod
    8L, so [u](A + T) carries [k]T exactly; reduced mod L it would accept or reject by the wrong multiple of T."""
    rs, arena, offs, orders = chain
    for pair in (False, True):
        for res in range(8):
            idx = rs.tors[res]
            codes, n_full = engine.debug_verify_prehashed(arena, rs.descs(idx, offs, SIG_DESC_DTYPE), pair=pair)
            assert codes.tolist() == rs.expected[idx].tolist(), (res, pair)
            assert n_full == 0
            accepted = sum(1 for i, c in zip(idx, codes) if c == 0 and rs.records[i].kind == "tors")
            assert accepted == {0: 8, 4: 4, 2: 2, 6: 2}.get(res, 1), (res, accepted)   # points T with [k]T = O


@pytest.mark.gpu
def test_device_routes_equal_model(engine, chain):
    """The device's own split of every chosen k routes as the model says (ok and the window count)."""
    rs = chain[0]
    ks = list(rs.routes)
    kb = np.frombuffer(b"".join(k.to_bytes(32, "little") for k in ks), dtype=np.uint8).reshape(-1, 32)
    dev = engine.debug_hs_split(kb)
    for j, k in enumerate(ks):
        rt = rs.routes[k]
        u = sum(int(dev[j, i]) << (32 * i) for i in range(5))
        v = sum(int(dev[j, 5 + i]) << (32 * i) for i in range(5))
        assert bool(dev[j, 10]) == rt.ok, hex(k)
        if rt.ok:
            assert (u, v, int(dev[j, 11]), int(dev[j, 12])) == (abs(rt.u), abs(rt.v), 0, int(rt.v < 0)), hex(k)
