"""The secp256k1 precompile path on the host (CPU only): the Python model
against public values and verdicts pinned by hand, the host library's Keccak,
recover, walk, record check and verdict against the model,
fdgpu_secp256k1_verify_host, the e = NULL block paths, the merge of the two
precompiles' verdicts, the size bound, the new header's ABI, and the sanitizer
program."""
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import pyref_precompile as pp
import pyref_secp256k1 as k1
from conftest import REPO
from firedancer_amd import _lib, tile, workload
from firedancer_amd import ed25519 as ed

DS, DO, SG, PF, NONE = k1.CODE_DATA_SIZE, k1.CODE_DATA_OFFSET, k1.CODE_SIGNATURE, k1.CODE_PARSE_FAIL, k1.NONE
KECCAK_LENS = (0, 1, 135, 136, 137, 271, 272, 998, 1062)     # 1062: the longest instruction data a transaction holds


@pytest.fixture(scope="module")
def cases():
    return k1.cases()


@pytest.fixture(scope="module")
def want(cases):
    return k1.expected(cases)


def info_tuple(r):
    return (int(r["instr_idx"]), int(r["rec_idx"]), int(r["ed_instr_cnt"]), int(r["sig_cnt"]), int(r["ed_code"]))


# ------------------------------------------------------------------ the model

def test_model_is_pinned_by_public_values():
    assert k1.keccak256(b"").hex() == "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"
    assert k1.keccak256(b"abc").hex() == "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"
    assert k1.on_curve(k1.G) and k1.mul(k1.N - 1, k1.G) == k1.neg(k1.G) and k1.add(k1.mul(k1.N - 1, k1.G), k1.G) is k1.INF
    assert k1.address(k1.G[0].to_bytes(32, "big") + k1.G[1].to_bytes(32, "big")).hex() == \
        "7e5f4552091a69125d5dfcb7b8c2659029395bdf"
    assert pp.b58decode32(pp.SECP256K1_NAME) == k1.SECP256K1_ID
    # the same sponge with SHA-3's padding byte is hashlib's SHA3-256: the permutation and the absorb over many
    # blocks are a public function's, and Keccak-256 differs from it in that one byte
    data = k1.Rng("sha3").bytes(1300)
    for n in KECCAK_LENS + (1232,):
        assert k1.keccak256(data[:n], 0x06) == hashlib.sha3_256(data[:n]).digest(), n
        assert k1.keccak256(data[:n]) != hashlib.sha3_256(data[:n]).digest()


def test_model_recovers_what_it_signed():
    """A chosen nonce: recover returns d G for s and, with the parity flipped, for n - s."""
    rng = k1.Rng("sign")
    for i in range(6):
        d, k, h = 1 + i * 0x1234567890ABCDEF, 0x9999 + i, rng.bytes(32)
        sig, recid = k1.sign(d, h, k)
        pub = k1.mul(d, k1.G)
        key = pub[0].to_bytes(32, "big") + pub[1].to_bytes(32, "big")
        assert k1.recover(h, sig, recid) == (0, key)
        hi = sig[:32] + (k1.N - int.from_bytes(sig[32:], "big")).to_bytes(32, "big")
        assert k1.recover(h, hi, recid ^ 1) == (0, key)
        rc, other = k1.recover(h, sig, recid ^ 1)
        assert rc == 0 and other != key


# verdicts worked out by hand from fd_precompiles.c:216-303, not by any code under test:
# name -> (code, failing instruction, failing record, secp256k1 instructions, records checked)
PINNED = {
    "no_instr": (0, NONE, NONE, 0, 0), "no_k1_instr": (0, NONE, NONE, 0, 0),
    "sz0": (DS, 0, NONE, 1, 0), "sz1_0": (0, NONE, NONE, 1, 0), "sz1_1": (DS, 0, NONE, 1, 0), "sz2_00": (DS, 0, NONE, 1, 0),
    "sz11": (DS, 1, NONE, 1, 0), "sz12": (0, NONE, NONE, 1, 1),
    "cnt0_sz12": (0, NONE, NONE, 1, 0), "cnt0_sz40": (0, NONE, NONE, 1, 0),      # without the feature: an empty table
    "cnt3_short": (DS, 1, NONE, 1, 0), "cnt3_exact": (0, NONE, NONE, 1, 3), "cnt3_over": (0, NONE, NONE, 1, 3),
    "cnt255": (DS, 1, NONE, 1, 0),
    "self_own0": (0, NONE, NONE, 1, 1), "self_own1": (0, NONE, NONE, 1, 1), "ix_later": (0, NONE, NONE, 1, 1),
    "ix_other_program_ed": (0, NONE, NONE, 1, 1), "ix_mixed": (0, NONE, NONE, 1, 1),
    "off_end_exact": (SG, 1, 0, 1, 1),          # resolves (offset + size == data_sz); the bytes there are no signature of the message
    "msg_sz_one_past": (SG, 1, 0, 1, 0), "msg_sz0": (0, NONE, NONE, 1, 1),
    "msg_sz0_at_end": (SG, 1, 0, 1, 1),         # resolves (offset == data_sz, size 0); the signature is over 40 bytes
    "msg_sz0_past_end": (SG, 1, 0, 1, 0), "msg_sz_ffff": (SG, 1, 0, 1, 0), "alias": (0, NONE, NONE, 1, 5),
    "order_recfail_then_badidx": (SG, 0, 0, 1, 1), "order_badidx_then_recfail": (DO, 0, 0, 1, 0),
    "order_recfail_then_badoff": (SG, 0, 0, 1, 1), "order_good_badoff_recfail": (SG, 0, 1, 1, 1),
    "order_sig_then_size": (SG, 0, 0, 2, 1), "order_good_then_size": (DS, 2, NONE, 2, 1),
    "order_size_then_more": (DS, 0, NONE, 3, 0), "order_idx_then_good": (DO, 0, 0, 2, 0),
    "ed_ignored": (0, NONE, NONE, 1, 1), "ed_only": (0, NONE, NONE, 0, 0), "id_last_account": (0, NONE, NONE, 1, 1),
    "id_near_miss": (0, NONE, NONE, 0, 0),
    "bad_recid": (SG, 0, 1, 1, 3), "bad_range": (SG, 0, 1, 1, 3), "bad_point": (SG, 0, 1, 1, 3), "bad_inf": (SG, 0, 1, 1, 3),
    "bad_addr": (SG, 0, 1, 1, 3), "bad_msg": (SG, 0, 1, 1, 3), "high_s": (0, NONE, NONE, 1, 2),
    "recid_2_3": (0, NONE, NONE, 1, 2), "lens_a": (0, NONE, NONE, 1, 5), "lens_b": (0, NONE, NONE, 1, 2),
    "long_998": (0, NONE, NONE, 1, 1), "long_1042": (0, NONE, NONE, 1, 1), "records_8": (SG, 0, 7, 1, 8),
    "v0": (0, NONE, NONE, 1, 1), "v0_lut": (SG, 0, 0, 1, 1),
    "max_records_1232": (SG, 0, 0, 1, 96), "max_records_400": (SG, 0, 0, 1, 20),
    "parse_trailing": (PF, NONE, NONE, 0, 0), "parse_truncated": (PF, NONE, NONE, 0, 0), "parse_empty": (PF, NONE, NONE, 0, 0),
}
# each resolve failing each way in each position p of a three-record table: the p records before it are checked
for _p in range(3):
    for _f in ("sig", "addr", "msg"):
        PINNED[f"res_{_f}_ixcnt_{_p}"] = (DO, 1, _p, 1, _p)
        PINNED[f"res_{_f}_onepast_{_p}"] = (SG, 1, _p, 1, _p)
        if _p == 1:
            PINNED[f"res_{_f}_ix255_{_p}"] = (DO, 1, _p, 1, _p)
            PINNED[f"res_{_f}_offffff_{_p}"] = (SG, 1, _p, 1, _p)
# the record code where a record's check fails
PINNED_RC = {"bad_recid": -1, "bad_range": -2, "bad_point": -3, "bad_inf": -4, "bad_addr": -5, "bad_msg": -5,
             "order_recfail_then_badidx": -5, "order_recfail_then_badoff": -2, "order_good_badoff_recfail": 0,
             "msg_sz_one_past": 0, "v0_lut": -2, "records_8": -5, "order_sig_then_size": -5}
# with libsecp256k1_fail_on_bad_count active (:230-235)
PINNED_FLAG = {"cnt0_sz12": (DS, 0, NONE, 1, 0), "cnt0_sz40": (DS, 1, NONE, 1, 0), "sz1_0": (0, NONE, NONE, 1, 0)}


def test_python_reference_gives_the_pinned_verdicts(cases, want):
    codes, infos, _ = want
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    assert set(PINNED) == set(names), set(PINNED) ^ set(names)
    for c, code, info in zip(cases, codes, infos):
        assert (int(code),) + info[:4] == PINNED[c.name], c.name
        if c.name in PINNED_RC:
            assert info[4] == PINNED_RC[c.name], c.name
        if int(code) != SG:
            assert info[4] == 0, c.name
    fc, fi, _ = k1.expected(cases, k1.FAIL_ON_BAD_COUNT)
    for c, code, info, code0, info0 in zip(cases, fc, fi, codes, infos):
        assert (int(code),) + info[:4] == PINNED_FLAG.get(c.name, (int(code0),) + info0[:4]), c.name
    for c in cases:
        assert (tile.txn_parse(c.payload)[0] != 0) == (c.model is not None), c.name
    for c in (0, DS, DO, SG, PF):
        assert c in codes.tolist()


# ----------------------------------------------------------- the host library

def test_host_keccak_matches_the_model():
    data = k1.Rng("keccak").bytes(1400)
    for n in KECCAK_LENS + (2, 134, 138, 270, 273, 407, 408, 409, 1232, 1359, 1360, 1361):
        assert tile.keccak256(data[:n]) == k1.keccak256(data[:n]), n
    assert tile.keccak256(b"abc").hex() == "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"


def test_host_recover_matches_the_model_on_the_edges():
    seen = set()
    for name, h, sig, recid in k1.recover_edges():
        exp = k1.recover(h, sig, recid)
        assert tile.secp256k1_recover(h, sig, recid) == exp, name
        seen.add(exp[0])
    assert seen == {0, -1, -2, -3, -4}
    rng = k1.Rng("recover")
    for i in range(40):                                        # arbitrary bytes: about half name a curve point
        h, sig, recid = rng.bytes(32), bytes(1) + rng.bytes(31) + bytes(1) + rng.bytes(31), rng.below(4)
        assert tile.secp256k1_recover(h, sig, recid) == k1.recover(h, sig, recid), i


def test_host_walk_matches_python(cases):
    for flags in (0, k1.FAIL_ON_BAD_COUNT):
        for c in cases:
            got = tile.secp256k1_walk(c.payload, flags)
            if c.model is None:
                assert got is None, c.name
                continue
            code, fi, fr, cnt, recs = k1.walk(*c.model, flags=flags)
            w, r = got
            assert (w["code"], w["instr_idx"], w["rec_idx"], w["ed_instr_cnt"], w["rec_cnt"]) == \
                (code, fi, fr, cnt, len(recs)), (c.name, flags)
            assert [tuple(int(x) for x in q) for q in r.tolist()] == recs, c.name


def test_walk_stores_no_more_than_its_cap(cases):
    by = {c.name: c for c in cases}
    for name in ("alias", "max_records_1232", "lens_a"):
        full_w, full = tile.secp256k1_walk(by[name].payload)
        n = full_w["rec_cnt"]
        assert n == len(full) >= 5
        for cap in (n, n - 1, 0):
            w, r = tile.secp256k1_walk(by[name].payload, rec_cap=cap)
            assert w == full_w and len(r) == cap and r.tolist() == full[:cap].tolist(), (name, cap)


def test_sig_bound_holds_and_is_tight(cases):
    for sz in list(range(0, 330)) + [399, 400, 1231, 1232, 1233, 5000, 1 << 40]:
        assert k1.sig_bound(sz) == _lib.lib().fdgpu_secp256k1_sig_bound(sz) == ed.secp256k1_sig_bound(sz), sz
    assert k1.sig_bound(1232) == 96 and k1.sig_bound(180) == 0 and k1.sig_bound(181) == 1
    assert k1.sig_bound(291) == 11 and k1.sig_bound(302) == 11 and k1.sig_bound(303) == 12      # the size's second byte
    g = k1.Gen("bound")
    extra = [k1.max_records(g, sz) for sz in list(range(236, 1233, 31)) + [291, 292, 302, 303, 304, 1232]]
    for c in list(cases) + extra:
        if c.model is None:
            continue
        n = len(k1.walk(*c.model)[4])
        assert n <= k1.sig_bound(len(c.payload)), c.name
        assert tile.secp256k1_walk(c.payload)[0]["rec_cnt"] == n
    for c in extra:       # tight wherever the table can hold a signature (65 bytes: 6 records)
        assert len(c.payload) == int(c.name.split("_")[-1])
        assert len(k1.walk(*c.model)[4]) == k1.sig_bound(len(c.payload)) >= 6, c.name


def test_host_record_and_verdict_match_python(cases, want):
    codes, infos, recs = want
    for c, code, info in zip(cases, codes, infos):
        if c.model is None:
            continue
        w, r = tile.secp256k1_walk(c.payload)
        pl = c.payload
        rc = [tile.secp256k1_record(pl, q) for q in r]
        assert rc == [k1.record_check(pl[m:m + ms], pl[s:s + 65], pl[a:a + 20]) for (_, _, s, a, m, ms) in recs[cases.index(c)]], c.name
        got, gi = tile.secp256k1_verdict(w, r, rc)
        assert (got, info_tuple(gi)) == (int(code), info), c.name
        assert bytes(gi["_pad"]) == bytes(7)
        if any(rc):       # checking every emitted record, rather than stopping at the first bad one, changes nothing
            k = next(i for i, e in enumerate(rc) if e)
            got2, gi2 = tile.secp256k1_verdict(w, r, rc[:k + 1] + [-3] * (len(rc) - k - 1))
            assert (got2, info_tuple(gi2)) == (got, info_tuple(gi)), c.name


def test_verify_host_and_block_host_path(cases, want):
    codes, infos, _ = want
    payloads = [c.payload for c in cases]
    for flags in (0, k1.FAIL_ON_BAD_COUNT):
        ec, ei, _ = (codes, infos, None) if not flags else k1.expected(cases, flags)
        got, gi = tile.secp256k1_verify_host(payloads, flags)
        assert got.tolist() == ec.tolist()
        assert [info_tuple(r) for r in gi] == ei
        # e = NULL: transactions without a secp256k1 instruction get 0 and report no position and no counts
        got, gi = tile.block_secp256k1_verify(None, payloads, flags, batch_txn_max=16)
        assert got.tolist() == ec.tolist()
        for c, r, info in zip(cases, gi, ei):
            assert info_tuple(r) == (info if info[2] else (NONE, NONE, 0, 0, 0)), c.name
    got, _ = tile.secp256k1_verify_host([])
    assert len(got) == 0
    got, _ = tile.block_secp256k1_verify(None, [])
    assert len(got) == 0


# ------------------------------------------------------------------ the merge

def _as_info(t, which=0):
    r = np.zeros(1, dtype=ed.PRECOMPILE_INFO_DTYPE)[0]
    r["instr_idx"], r["rec_idx"], r["ed_instr_cnt"], r["sig_cnt"], r["ed_code"] = t[:5]
    return r


def test_merge_matches_python_and_the_rules(oracle):
    block = k1.mixed_block(workload.sign)
    e_codes, e_infos, _ = pp.expected(block, oracle.verify)
    k_codes, k_infos, _ = k1.expected(block)
    by = {}
    for c, ec, ei, kc, ki in zip(block, e_codes, e_infos, k_codes, k_infos):
        exp = k1.merge((int(ec), ei), (int(kc), ki))
        code, info = tile.precompile_merge(int(ec), _as_info(ei), int(kc), _as_info(ki))
        assert (code, info_tuple(info) + (int(info["_pad"][0]),)) == exp, c.name
        by[c.name] = exp
    # worked by hand: the failure at the smaller instruction wins, whichever program it is
    assert by["both_ok"][0] == 0 and by["both_ok"][1][:2] == (NONE, NONE) and by["both_ok"][1][5] == 0
    assert (by["ed_fails_first"][0], by["ed_fails_first"][1][0], by["ed_fails_first"][1][5]) == (SG, 0, 1)
    assert (by["k1_fails_first"][0], by["k1_fails_first"][1][0], by["k1_fails_first"][1][4:]) == (SG, 0, (-5, 2))
    assert (by["only_ed_fails"][0], by["only_ed_fails"][1][0], by["only_ed_fails"][1][5]) == (SG, 1, 1)
    assert (by["only_k1_fails"][0], by["only_k1_fails"][1][0], by["only_k1_fails"][1][4:]) == (SG, 2, (-1, 2))
    assert (by["k1_size_before_ed_sig"][0], by["k1_size_before_ed_sig"][1][0], by["k1_size_before_ed_sig"][1][5]) == (DS, 0, 2)
    assert (by["ed_size_before_k1_sig"][0], by["ed_size_before_k1_sig"][1][0], by["ed_size_before_k1_sig"][1][5]) == (DS, 0, 1)
    assert by["parse_fail"][0] == PF and by["neither"][0] == 0
    # PARSE_FAIL stays, CAP on either side is CAP, both with no position
    none = (NONE, NONE, 0, 0, 0)
    for a, b, exp in ((PF, 0, PF), (0, PF, PF), (k1.CODE_CAP, 0, k1.CODE_CAP), (SG, k1.CODE_CAP, k1.CODE_CAP),
                      (k1.CODE_CAP, PF, PF)):
        ia = (3, 1, 1, 2, -1) if a == SG else none
        code, info = tile.precompile_merge(a, _as_info(ia), b, _as_info(none))
        assert code == exp == k1.merge((a, ia), (b, none))[0] and info_tuple(info) == none


def test_block_verify_all_host_path(oracle):
    def fn(a, t):
        return [oracle.verify(bytes(a[int(x["msg_off"]):int(x["msg_off"]) + int(x["msg_sz"])]),
                              bytes(a[int(x["sig_off"]):int(x["sig_off"]) + 64]),
                              bytes(a[int(x["pub_off"]):int(x["pub_off"]) + 32])) for x in t]
    block = k1.mixed_block(workload.sign)
    e_codes, e_infos, _ = pp.expected(block, oracle.verify)
    k_codes, k_infos, _ = k1.expected(block)
    got, gi = tile.block_precompile_verify_all(None, [c.payload for c in block], host_verifier=tile.PyVerifier(fn))
    for c, g, r, ec, ei, kc, ki in zip(block, got, gi, e_codes, e_infos, k_codes, k_infos):
        none = (NONE, NONE, 0, 0, 0)
        # a transaction a block function does not forward reports no position and no counts
        exp = k1.merge((int(ec), ei if ei[2] else none), (int(kc), ki if ki[2] else none))
        assert (int(g), info_tuple(r) + (int(r["_pad"][0]),)) == exp, c.name
    with pytest.raises(RuntimeError):
        tile.block_precompile_verify_all(None, [c.payload for c in block])      # the Ed25519 host path needs a verifier


# ------------------------------------------------------------------ the header

def test_secp256k1_header_abi():
    hdr = _lib.SECP256K1_HEADER_PATH
    src = (f'#include "{hdr}"\n'
           '_Static_assert(FDGPU_SECP256K1_FAIL_ON_BAD_COUNT == 1u, "flag");\n'
           'int main(void){ fdgpu_precompile_t s; (void)s; return FDGPU_SECP256K1_ERR_RECID + 1 + FDGPU_SECP256K1_ERR_RANGE + 2 + '
           'FDGPU_SECP256K1_ERR_POINT + 3 + FDGPU_SECP256K1_ERR_INFINITY + 4 + FDGPU_SECP256K1_ERR_ADDRESS + 5 + '
           'FDGPU_CODE_PRECOMPILE_SIGNATURE + 72; }\n')
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-x", "c", "-", "-fsyntax-only"], input=src,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    code = re.sub(r"/\*.*?\*/", "", open(hdr).read(), flags=re.S)
    assert set(re.findall(r"#include\s*[<\"]([^>\"]+)", code)) == {"stddef.h", "stdint.h", "fd_precompile_gpu.h"}
    names = _lib.header_functions(hdr)
    assert names == ["fdgpu_debug_keccak256", "fdgpu_debug_secp256k1_recover", "fdgpu_debug_secp256k1_time",
                     "fdgpu_debug_secp256k1_walk", "fdgpu_poll_secp256k1", "fdgpu_secp256k1_sig_bound",
                     "fdgpu_submit_secp256k1"]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for n in names + ["fdgpu_debug_secp256k1_ops"]:            # the last is csrc/fdgpu_secp256k1.h's, not a public header's
        assert re.search(r"\sT\s" + n + r"$", out, flags=re.M), n
    for h in (_lib.HEADER_PATH, _lib.PRECOMPILE_HEADER_PATH, hdr):
        assert "fdgpu_debug_secp256k1_ops" not in open(h).read()
    # the older headers keep their lists and point here
    assert len(_lib.header_functions()) == 51
    assert len(_lib.header_functions(_lib.PRECOMPILE_HEADER_PATH)) == 5
    text = open(_lib.PRECOMPILE_HEADER_PATH).read()
    assert "secp256k1" in text and "fd_secp256k1_gpu.h" in text
    tout = subprocess.run(["nm", "-D", "--defined-only", tile.TILE_LIB_PATH], capture_output=True, text=True,
                          check=True).stdout
    for n in ("fdt_keccak256", "fdt_secp256k1_recover", "fdt_secp256k1_walk", "fdt_secp256k1_record", "fdt_secp256k1_verdict",
              "fdgpu_secp256k1_verify_host", "fdgpu_block_secp256k1_verify", "fdgpu_precompile_merge",
              "fdgpu_block_precompile_verify_all"):
        assert re.search(r"\sT\s" + n + r"$", tout, flags=re.M), n
        assert n in tile.header_functions()
    assert (ed.SECP256K1_ERR_RECID, ed.SECP256K1_ERR_RANGE, ed.SECP256K1_ERR_POINT, ed.SECP256K1_ERR_INFINITY,
            ed.SECP256K1_ERR_ADDRESS, ed.SECP256K1_FAIL_ON_BAD_COUNT) == (-1, -2, -3, -4, -5, 1)
    internal = open(os.path.join(REPO, "firedancer_amd", "csrc", "fdgpu_secp256k1.h")).read()
    assert f"FDGPU_SECP256K1_OPS_IN  {ed.SECP256K1_OPS_IN}u" in internal and f"FDGPU_SECP256K1_OPS_OUT {ed.SECP256K1_OPS_OUT}u" in internal


def test_sanitizer_program(tmp_path, cases):
    """tools/secp256k1_san.cpp under ASan + UBSan: the Keccak and the recover
    over vectors, the parse, the walk, the record checks and the verdict over
    the case set, and 50,000 mutated payloads (300 of their records checked),
    each buffer in an allocation of its exact size."""
    exe = tmp_path / "secp256k1_san"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", "-I", os.path.join(REPO, "include"),
                        os.path.join(REPO, "tools", "secp256k1_san.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    n_cases = 0
    with open(tmp_path / "cases.bin", "wb") as f:   # [u32 size][u8 flags][i8 verdict][i8 record code][u16 records][bytes]
        for flags in (0, k1.FAIL_ON_BAD_COUNT):
            codes, infos, _ = k1.expected(cases, flags)
            for c, code, info in zip(cases, codes, infos):
                if flags and c.name not in PINNED_FLAG:
                    continue
                f.write(len(c.payload).to_bytes(4, "little") + bytes([flags]) + int(code).to_bytes(1, "little", signed=True) +
                        int(info[4]).to_bytes(1, "little", signed=True) + info[3].to_bytes(2, "little") + c.payload)
                n_cases += 1
    data = k1.Rng("san").bytes(1400)
    edges = k1.recover_edges()
    with open(tmp_path / "vectors.bin", "wb") as f:
        for n in KECCAK_LENS + (1232,):
            f.write(b"\1" + n.to_bytes(4, "little") + data[:n] + k1.keccak256(data[:n]))
        for _, h, sig, recid in edges:
            rc, key = k1.recover(h, sig, recid)
            f.write(b"\2" + h + sig + bytes([recid]) + rc.to_bytes(1, "little", signed=True) + key)
    r = subprocess.run([str(exe), str(tmp_path / "cases.bin"), str(tmp_path / "vectors.bin"), "50000", "300"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    m = re.search(r"vectors (\d+) keccak, (\d+) recover ok; cases (\d+) ok, random (\d+): (\d+) parsed, (\d+) records, (\d+) checked",
                  r.stdout)
    assert m, r.stdout
    assert [int(x) for x in m.groups()[:4]] == [len(KECCAK_LENS) + 1, len(edges), n_cases, 50000], r.stdout
    assert int(m.group(5)) > 10000 and int(m.group(6)) > 10000 and int(m.group(7)) == 300, r.stdout
