"""The PoH check on the host: the hashlib model against the reference's golden
vectors, the tile library's host path (fdgpu_poh_verify_host) against the
model, the block-level caller with no engine, and the argument errors."""
import numpy as np
import pytest

import pyref_poh as pp
from conftest import load_json
from firedancer_amd import tile, workload
from firedancer_amd.ed25519 import (CODE_POH_MISMATCH, CODE_POH_TOO_LONG, POH_DTYPE, POH_HASH_CNT_MAX, POH_NO_MIX,
                                    poh_chunk)

CAP = 1 << 16


@pytest.fixture(scope="module")
def vectors():
    return load_json("poh_vectors.json")["vectors"]


def sigs_of(payload):
    fp, raw = tile.txn_parse(payload)
    assert fp
    h = tile.txn_decode(raw)
    return [payload[h["signature_off"] + 64 * k: h["signature_off"] + 64 * k + 64] for k in range(h["signature_cnt"])]


@pytest.fixture(scope="module")
def stream():
    arena, txns, _ = workload.cfg3(64, seed=77)
    return pp.stream(np.random.default_rng(5), workload.payloads(arena, txns), sigs_of)


def test_model_reproduces_the_golden_vectors(vectors):
    assert [v["name"] for v in vectors] == ["Solana mainnet block 0", "Solana mainnet block 1"]
    for v in vectors:
        h = bytes.fromhex(v["pre"])
        for s in v["steps"]:
            h = pp.append(h, s["append"]) if "append" in s else pp.mixin(h, bytes.fromhex(s["mixin"]))
        assert h.hex() == v["post"], v["name"]
    t = load_json("bmtree_vectors.json")["tree32"]
    assert (t["hash_sz"], t["prefix_sz"], len(t["leaves"])) == (32, 1, 11)
    assert pp.fold([pp.leaf(s.encode()) for s in t["leaves"]]).hex() == t["root"]


def test_host_path_matches_the_model_on_the_matrix():
    chunk = poh_chunk()
    assert 2 <= chunk <= 4096
    arena, entries, sig_offs = pp.matrix(chunk, np.random.default_rng(3)).arrays()
    assert len(entries) == 8 * (2 + len(pp.SIG_CNTS))
    assert {int(o) % 16 for o in sig_offs} == set(range(16))
    assert (entries["prev_off"] % 2 == 1).all() and (entries["hash_off"] % 2 == 1).all()
    want_codes, want_hashes = pp.evaluate(arena, entries, sig_offs, CAP)
    assert not want_codes.any()
    codes, hashes = tile.poh_verify_host(arena, entries, sig_offs, CAP)
    assert codes.tolist() == want_codes.tolist()
    assert (hashes == want_hashes).all()
    # spoiled entries, and a cap that cuts the longest chains off
    rng = np.random.default_rng(4)
    bad = {5: "hash", 9: "prev", 17: "sig", 40: "cnt+", 60: "cnt-", 77: "sig"}
    for i, how in bad.items():
        if how in ("sig",) and not entries["sig_cnt"][i]:
            how = "hash"
        pp.corrupt(arena, entries, sig_offs, i, how, rng)
    want_codes, want_hashes = pp.evaluate(arena, entries, sig_offs, chunk)
    assert set(np.flatnonzero(want_codes == CODE_POH_MISMATCH)) >= set(bad) - set(np.flatnonzero(entries["hash_cnt"] > chunk))
    assert (want_codes == CODE_POH_TOO_LONG).sum() >= 2 * (2 + len(pp.SIG_CNTS)) - 2
    codes, hashes = tile.poh_verify_host(arena, entries, sig_offs, chunk)
    assert codes.tolist() == want_codes.tolist()
    assert (hashes == want_hashes).all()
    assert not hashes[codes == CODE_POH_TOO_LONG].any()


def test_host_path_runs_mainnet_block_0(vectors):
    """one chain of 800,000 hashes, the cap at the ceiling"""
    b, last = pp.golden_entries(vectors[0])
    arena, entries, sig_offs = b.arrays()
    assert len(entries) == 1 and entries["hash_cnt"][0] == 800000 and last.hex() == vectors[0]["post"]
    codes, hashes = tile.poh_verify_host(arena, entries, sig_offs, POH_HASH_CNT_MAX)
    assert codes.tolist() == [0] and hashes[0].tobytes().hex() == vectors[0]["post"]
    codes, hashes = tile.poh_verify_host(arena, entries, sig_offs, 799999)
    assert codes.tolist() == [CODE_POH_TOO_LONG] and not hashes.any()


def test_block_caller_on_the_host(stream):
    s = stream
    m = len(s["hash_cnt"])
    assert m == 24 and sum(s["txn_cnt"]) == len(s["payloads"]) and sum(1 for c in s["txn_cnt"] if c) >= 9

    def run(st, **kw):
        return tile.block_poh_verify(None, st["in_hash"], st["hash_cnt"], st["entry_hash"], st["txn_cnt"], st["payloads"],
                                     CAP, **kw).tolist()

    assert run(s) == [0] * m
    assert run(s, batch_entry_max=5) == [0] * m
    # entries chain from the claimed hashes: a wrong start fails entry 0 alone
    assert run(dict(s, in_hash=bytes(32))) == [CODE_POH_MISMATCH] + [0] * (m - 1)
    # one corrupted entry fails alone, its successor still passes
    for k in (3, 8):
        hc = list(s["hash_cnt"]); hc[k] += 1
        want = [0] * m; want[k] = CODE_POH_MISMATCH
        assert run(dict(s, hash_cnt=hc)) == want, k
    eh = list(s["entry_hash"]); eh[6] = bytes([eh[6][0] ^ 1]) + eh[6][1:]
    want = [0] * m; want[6] = want[7] = CODE_POH_MISMATCH       # 7 starts from the spoiled claim, 8 from 7's own
    assert run(dict(s, entry_hash=eh)) == want
    # an unparseable transaction: its entry only
    k = next(i for i, c in enumerate(s["txn_cnt"]) if c >= 2)
    j = sum(s["txn_cnt"][:k]) + 1
    ps = list(s["payloads"]); ps[j] = b"\x00" * 40
    want = [0] * m; want[k] = tile.REPLAY_PARSE_FAIL
    assert run(dict(s, payloads=ps)) == want
    # an entry above the cap
    hc = list(s["hash_cnt"]); hc[10] = CAP + 1
    want = [0] * m; want[10] = CODE_POH_TOO_LONG
    assert run(dict(s, hash_cnt=hc)) == want
    with pytest.raises(RuntimeError):                             # the txn counts do not sum to the payloads
        run(dict(s, txn_cnt=[c + (i == 0) for i, c in enumerate(s["txn_cnt"])]))
    with pytest.raises(RuntimeError):
        tile.block_poh_verify(None, s["in_hash"], s["hash_cnt"], s["entry_hash"], s["txn_cnt"], s["payloads"], 0)


def test_host_path_argument_errors():
    """every FDGPU_ERR_INVAL case of fdgpu_submit_poh that does not need an engine's limits"""
    arena, entries, sig_offs = pp.mixed(12, np.random.default_rng(8), hi=20).arrays()
    assert entries["sig_cnt"].any() and (entries["mix_off"] != POH_NO_MIX).any()
    tile.poh_verify_host(arena, entries, sig_offs, 20)

    def bad(en=entries, so=sig_offs, cap=20, a=arena):
        with pytest.raises(RuntimeError, match="-10"):
            tile.poh_verify_host(a, en, so, cap)

    for f in ("prev_off", "hash_off"):
        e = entries.copy(); e[f][4] = len(arena) - 31
        bad(e)
    k = int(np.flatnonzero(entries["mix_off"] != POH_NO_MIX)[0])
    e = entries.copy(); e["mix_off"][k] = len(arena) - 31
    bad(e)
    e = entries.copy(); e["sig_cnt"][k] = 1; e["sig_first"][k] = 0
    bad(e)                                                        # mix_off together with sig_cnt
    k = int(np.flatnonzero(entries["sig_cnt"])[-1])
    e = entries.copy(); e["sig_cnt"][k] += 1
    bad(e)                                                        # signatures outside sig_offs
    i, j = np.flatnonzero(entries["sig_cnt"])[:2]
    e = entries.copy(); e["sig_first"][j] = e["sig_first"][i] + e["sig_cnt"][i] - 1
    bad(e)                                                        # two ranges share a signature
    e = entries.copy(); e["sig_first"][j], e["sig_cnt"][j] = e["sig_first"][i], e["sig_cnt"][i]
    bad(e)                                                        # the same range twice
    e = entries.copy(); e["sig_first"][i], e["sig_first"][j] = entries["sig_first"][j], entries["sig_first"][i]
    e["sig_cnt"][i] = e["sig_cnt"][j] = 1
    bad(e)                                                        # disjoint, but not ascending
    so = sig_offs.copy(); so[0] = len(arena) - 63
    bad(so=so)
    bad(cap=0)
    bad(cap=POH_HASH_CNT_MAX + 1)
    assert tile.poh_verify_host(arena, entries[:0], sig_offs[:0], 20)[0].tolist() == []


def test_an_entry_given_twice_brings_its_offsets_twice():
    """The device folds each signature range in place, so ranges may not be shared; the same microblock twice in a
    batch (here with two claims, one of them wrong) repeats its offsets in sig_offs and gets the model's answers."""
    b = pp.Batch(np.random.default_rng(9))
    b.add(30, n_sig=5)
    arena, entries, sig_offs = b.arrays()
    twice = np.concatenate([entries, entries])
    with pytest.raises(RuntimeError, match="-10"):
        tile.poh_verify_host(arena, twice, sig_offs, CAP)
    twice["sig_first"][1] = len(sig_offs)
    twice["hash_cnt"][1] += 1
    so = np.concatenate([sig_offs, sig_offs])
    want = pp.evaluate(arena, twice, so, CAP)
    assert want[0].tolist() == [0, CODE_POH_MISMATCH]
    codes, hashes = tile.poh_verify_host(arena, twice, so, CAP)
    assert codes.tolist() == want[0].tolist() and (hashes == want[1]).all()


def test_poh_header_abi():
    import re
    import subprocess
    from firedancer_amd import _lib
    hdr = _lib.POH_HEADER_PATH
    src = (f'#include "{hdr}"\n_Static_assert(sizeof(fdgpu_poh_entry_t) == 32, "entry");\n'
           'int main(void){ fdgpu_poh_entry_t e; (void)e; return FDGPU_CODE_POH_MISMATCH + FDGPU_CODE_POH_TOO_LONG + 137; }\n')
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-x", "c", "-", "-fsyntax-only"], input=src,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names = _lib.header_functions(hdr)
    assert names == sorted(["fdgpu_submit_poh", "fdgpu_poll_poh", "fdgpu_poh_limits", "fdgpu_poh_chunk",
                            "fdgpu_debug_poh", "fdgpu_debug_poh_time"]), names
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for n in names:
        assert re.search(r"\sT\s" + n + r"$", out, flags=re.M), n
    assert POH_DTYPE.itemsize == 32 and POH_DTYPE.fields["mix_off"][1] == 24
    assert (CODE_POH_MISMATCH, CODE_POH_TOO_LONG, POH_NO_MIX, POH_HASH_CNT_MAX) == (-68, -69, 0xFFFFFFFF, 1 << 20)
    tout = subprocess.run(["nm", "-D", "--defined-only", tile.TILE_LIB_PATH], capture_output=True, text=True,
                          check=True).stdout
    for n in ("fdgpu_poh_verify_host", "fdgpu_block_poh_verify"):
        assert re.search(r"\sT\s" + n + r"$", tout, flags=re.M), n
