"""The Ed25519 precompile path on the host (CPU only): the Python reference
against verdicts pinned by hand, the host library's walk and verdict against
the Python reference, fdgpu_precompiles_verify and
fdgpu_block_precompile_verify(e = NULL) over the oracle, the size bound, the
new header's ABI, and the sanitizer program."""
import os
import re
import subprocess

import numpy as np
import pytest

import pyref_precompile as pp
from conftest import REPO
from firedancer_amd import _lib, tile, workload

DS, DO, SG, PF, NONE = pp.CODE_DATA_SIZE, pp.CODE_DATA_OFFSET, pp.CODE_SIGNATURE, pp.CODE_PARSE_FAIL, pp.NONE


@pytest.fixture(scope="module")
def cases():
    return pp.cpu_cases(workload.sign)


@pytest.fixture(scope="module")
def want(cases, oracle):
    return pp.expected(cases, oracle.verify)


def oracle_fn(oracle):
    def fn(a, t):
        return [oracle.verify(bytes(a[int(x["msg_off"]):int(x["msg_off"]) + int(x["msg_sz"])]),
                              bytes(a[int(x["sig_off"]):int(x["sig_off"]) + 64]),
                              bytes(a[int(x["pub_off"]):int(x["pub_off"]) + 32])) for x in t]
    return fn


def info_tuple(r):
    return (int(r["instr_idx"]), int(r["rec_idx"]), int(r["ed_instr_cnt"]), int(r["sig_cnt"]), int(r["ed_code"]))


def test_program_id_from_base58(cases):
    """The id the rules compare is the base58 name decoded here, and the host
    walk counts exactly the instructions of that program."""
    assert pp.b58decode32(pp.ED25519_NAME).hex() == pp.ED25519_ID_HEX
    assert pp.b58decode32("11111111111111111111111111111111") == bytes(32)
    by = {c.name: c for c in cases}
    assert tile.precompile_walk(by["sz2_00"].payload)[0]["ed_instr_cnt"] == 1
    assert tile.precompile_walk(by["id_near_miss"].payload)[0]["ed_instr_cnt"] == 0
    assert tile.precompile_walk(by["id_last_account"].payload)[0]["ed_instr_cnt"] == 1
    assert tile.precompile_walk(by["secp_only"].payload)[0]["ed_instr_cnt"] == 0


# verdicts worked out by hand from fd_precompiles.c:121-206, not by any code under test:
# name -> (code, failing instruction, failing record, Ed25519 instructions, records verified)
PINNED = {
    "no_instr": (0, NONE, NONE, 0, 0), "no_ed_instr": (0, NONE, NONE, 0, 0),
    "sz0": (DS, 0, NONE, 1, 0), "sz1": (DS, 0, NONE, 1, 0), "sz2_00": (0, NONE, NONE, 1, 0),
    "sz2_0x": (0, NONE, NONE, 1, 0), "sz2_10": (DS, 0, NONE, 1, 0), "sz15": (DS, 1, NONE, 1, 0),
    "sz16": (0, NONE, NONE, 1, 1), "sz16_pad_ignored": (0, NONE, NONE, 1, 1), "cnt0_sz16": (DS, 1, NONE, 1, 0),
    "cnt0_sz40": (DS, 0, NONE, 1, 0), "cnt3_short": (DS, 1, NONE, 1, 0), "cnt3_exact": (0, NONE, NONE, 1, 3),
    "cnt3_over": (0, NONE, NONE, 1, 3), "cnt255": (DS, 1, NONE, 1, 0),
    "self_ffff": (0, NONE, NONE, 1, 1), "self_own0": (0, NONE, NONE, 1, 1), "self_own1": (0, NONE, NONE, 1, 1),
    "ix_sig_ffff": (0, NONE, NONE, 1, 1), "ix_sig_own": (0, NONE, NONE, 1, 1), "ix_sig_cnt": (DO, 0, 0, 1, 0),
    "ix_sig_cnt1": (DO, 0, 0, 1, 0), "ix_sig_fffe": (DO, 0, 0, 1, 0),
    "ix_pub_ffff": (0, NONE, NONE, 1, 1), "ix_pub_own": (0, NONE, NONE, 1, 1), "ix_pub_cnt": (DO, 0, 0, 1, 0),
    "ix_pub_cnt1": (DO, 0, 0, 1, 0), "ix_pub_fffe": (DO, 0, 0, 1, 0), "ix_msg_fffe": (DO, 0, 0, 1, 0),
    "msg_sz0_at_end": (SG, 1, 0, 1, 1),         # resolves (offset == data_sz, size 0); the signature is over 40 bytes
    "ix_msg_ffff": (0, NONE, NONE, 1, 1), "ix_msg_own": (0, NONE, NONE, 1, 1), "ix_msg_cnt": (DO, 0, 0, 1, 0),
    "ix_msg_cnt1": (DO, 0, 0, 1, 0),
    "ix_earlier": (0, NONE, NONE, 1, 1), "ix_later": (0, NONE, NONE, 1, 1), "ix_other_program_secp": (0, NONE, NONE, 1, 1),
    "ix_mixed": (0, NONE, NONE, 1, 1),
    "off_end_exact": (SG, 1, 0, 1, 1),          # resolves (offset + size == data_sz); the bytes there are no signature
    "off_sig_one_past": (DO, 1, 0, 1, 0), "off_pub_one_past": (DO, 1, 0, 1, 0), "off_msg_one_past": (DO, 1, 0, 1, 0),
    "off_sig_ffff": (DO, 1, 0, 1, 0), "off_pub_ffff": (DO, 1, 0, 1, 0), "off_msg_ffff": (DO, 1, 0, 1, 0),
    "msg_sz_one_past": (DO, 1, 0, 1, 0), "msg_sz0": (0, NONE, NONE, 1, 1), "msg_sz0_past_end": (DO, 1, 0, 1, 0),
    "msg_sz_ffff": (DO, 1, 0, 1, 0), "alias": (0, NONE, NONE, 1, 5),
    "order_badsig_then_badoff": (SG, 0, 0, 1, 1), "order_good_badoff_badsig": (DO, 0, 1, 1, 1),
    "order_sig_then_size": (SG, 0, 0, 2, 1), "order_good_then_size": (DS, 2, NONE, 2, 1),
    "order_size_then_more_ed": (DS, 0, NONE, 3, 0), "order_off_then_good": (DO, 0, 0, 2, 0),
    "secp_ignored": (0, NONE, NONE, 1, 1), "secp_only": (0, NONE, NONE, 0, 0), "id_last_account": (0, NONE, NONE, 1, 1),
    "id_near_miss": (0, NONE, NONE, 0, 0), "bad_S": (SG, 0, 1, 1, 3), "bad_key": (SG, 0, 1, 1, 3),
    "bad_R": (SG, 0, 1, 1, 3), "bad_msg": (SG, 0, 1, 1, 3), "lens_a": (0, NONE, NONE, 1, 5), "lens_b": (0, NONE, NONE, 1, 4),
    "long_msg": (0, NONE, NONE, 1, 1), "records_8": (SG, 0, 7, 1, 8), "v0": (0, NONE, NONE, 1, 1),
    "v0_lut": (SG, 0, 0, 1, 1), "max_records_1232": (SG, 0, 0, 1, 75), "max_records_400": (SG, 0, 0, 1, 16),
    "parse_trailing": (PF, NONE, NONE, 0, 0), "parse_truncated": (PF, NONE, NONE, 0, 0),
    "parse_empty": (PF, NONE, NONE, 0, 0), "parse_sig_cnt0": (PF, NONE, NONE, 0, 0),
}


def test_python_reference_gives_the_pinned_verdicts(cases, want):
    codes, infos, _ = want
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    missing = set(PINNED) - set(names)
    assert not missing, missing
    for c, code, info in zip(cases, codes, infos):
        if c.name in PINNED:
            assert (int(code),) + info[:4] == PINNED[c.name], c.name
    assert len(PINNED) >= len(cases) - 4          # the few unpinned ones are variants of pinned ones
    # every parsing case parses in the host library too, and the others do not
    for c in cases:
        assert (tile.txn_parse(c.payload)[0] != 0) == (c.model is not None), c.name


def test_ed_codes_are_the_oracles(cases, want, oracle):
    """bad S, a small-order key, another R: ed_code is what fd_ed25519_verify
    returns for that record, and all three error codes occur."""
    codes, infos, recs = want
    by = {c.name: i for i, c in enumerate(cases)}
    seen = set()
    for bad in ("S", "key", "R", "msg"):
        i = by[f"bad_{bad}"]
        j, r, s, p, m, ms = recs[i][1]
        pl = cases[i].payload
        ed = oracle.verify(pl[m:m + ms], pl[s:s + 64], pl[p:p + 32])
        assert ed in (-1, -2, -3) and infos[i][4] == ed and codes[i] == SG
        seen.add(ed)
    assert seen == {-1, -2, -3}


def test_host_walk_matches_python(cases):
    for c in cases:
        got = tile.precompile_walk(c.payload)
        if c.model is None:
            assert got is None, c.name
            continue
        code, fi, fr, ed_cnt, recs = pp.walk(*c.model)
        w, r = got
        assert (w["code"], w["instr_idx"], w["rec_idx"], w["ed_instr_cnt"], w["rec_cnt"]) == \
            (code, fi, fr, ed_cnt, len(recs)), c.name
        assert [tuple(int(x) for x in q) for q in r.tolist()] == recs, c.name


def test_walk_stores_no_more_than_its_cap(cases):
    """rec_cap exact, one short and zero: the count is the same, and nothing
    is stored past the cap (the array handed over holds exactly cap records).
    This is all the CPU has of `sig_cap`: the host path has no cap and no
    FDGPU_CODE_PRECOMPILE_CAP, so the code itself -- exact, one short, at the
    size bound -- is checked only on the GPU
    (tests/test_gpu_precompile.py::test_caps_and_limits)."""
    by = {c.name: c for c in cases}
    for name in ("alias", "max_records_1232", "lens_a"):
        full_w, full = tile.precompile_walk(by[name].payload)
        n = full_w["rec_cnt"]
        assert n == len(full) >= 5
        for cap in (n, n - 1, 0):
            w, r = tile.precompile_walk(by[name].payload, rec_cap=cap)
            assert w == full_w and len(r) == cap and r.tolist() == full[:cap].tolist(), (name, cap)


def test_sig_bound_holds_and_is_tight(cases):
    for sz in list(range(0, 260)) + [399, 400, 1231, 1232, 1233, 5000, 1 << 40]:
        assert pp.sig_bound(sz) == _lib.lib().fdgpu_precompile_sig_bound(sz), sz
    assert pp.sig_bound(1232) == 75 and pp.sig_bound(184) == 0 and pp.sig_bound(185) == 1
    g = pp.Gen(workload.sign, "bound")
    extra = [pp.random_txn(g, n) for n in (0, 1, 2, 17, 64)] + [pp.random_txn(g, 64, bad_at=63)] + [pp.max_records(g, sz) for sz in list(range(241, 1233, 37)) + [1232]]
    for c in list(cases) + extra:
        if c.model is None:
            continue
        n = len(pp.walk(*c.model)[4])
        assert n <= pp.sig_bound(len(c.payload)), c.name
        assert tile.precompile_walk(c.payload)[0]["rec_cnt"] == n
    for c in extra[6:]:
        assert len(pp.walk(*c.model)[4]) == pp.sig_bound(len(c.payload)) >= 1, c.name      # tight wherever the table can hold a signature (5 records)


def test_host_verdict_matches_python(cases, want, oracle):
    codes, infos, recs = want
    for c, code, info in zip(cases, codes, infos):
        if c.model is None:
            continue
        w, r = tile.precompile_walk(c.payload)
        pl = c.payload
        ed = [oracle.verify(pl[int(q["msg_off"]):int(q["msg_off"]) + int(q["msg_sz"])],
                            pl[int(q["sig_off"]):int(q["sig_off"]) + 64], pl[int(q["pub_off"]):int(q["pub_off"]) + 32])
              for q in r]
        got, gi = tile.precompile_verdict(w, r, ed)
        assert (got, info_tuple(gi)) == (int(code), info), c.name
        assert bytes(gi["_pad"]) == bytes(7)
        # verifying every emitted record, rather than stopping at the first bad one, changes nothing: make the
        # records behind the first failure fail too
        if any(ed):
            k = next(i for i, e in enumerate(ed) if e)
            got2, gi2 = tile.precompile_verdict(w, r, ed[:k + 1] + [-3] * (len(ed) - k - 1))
            assert (got2, info_tuple(gi2)) == (got, info_tuple(gi)), c.name


def test_precompiles_verify_over_the_oracle(cases, want, oracle):
    codes, infos, recs = want
    ver = tile.PyVerifier(oracle_fn(oracle))
    got, gi = tile.precompiles_verify(ver, [c.payload for c in cases], batch_max=50)
    assert got.tolist() == codes.tolist()
    assert [info_tuple(r) for r in gi] == infos
    assert sum(ver.batches) == sum(len(r) for r in recs) and len(ver.batches) >= 4 and max(ver.batches) <= 50
    for c in (0, DS, DO, SG, PF):
        assert c in codes.tolist(), c
    # an empty block, and a verifier that fails
    got, gi = tile.precompiles_verify(ver, [])
    assert len(got) == 0
    bad = tile.PyVerifier(oracle_fn(oracle), slots=0)
    with pytest.raises(RuntimeError):
        tile.precompiles_verify(bad, [cases[16].payload for _ in range(3)] + [c.payload for c in cases])


def test_block_precompile_verify_host_path(cases, want, oracle):
    """e = NULL: transactions without an Ed25519 instruction get 0 and never
    reach the verifier, unparseable ones PARSE_FAIL, the rest the host path."""
    codes, infos, recs = want
    ver = tile.PyVerifier(oracle_fn(oracle))
    payloads = [c.payload for c in cases]
    got, gi = tile.block_precompile_verify(None, payloads, batch_txn_max=64, host_verifier=ver)
    assert got.tolist() == codes.tolist()
    for c, r, info in zip(cases, gi, infos):
        # a transaction that is not forwarded reports no position and no counts
        assert info_tuple(r) == (info if info[2] else (NONE, NONE, 0, 0, 0)), c.name
    assert sum(ver.batches) == sum(len(r) for r in recs)
    with pytest.raises(RuntimeError):
        tile.block_precompile_verify(None, payloads)            # the host path needs a verifier


def test_precompile_header_abi():
    hdr = _lib.PRECOMPILE_HEADER_PATH
    src = (f'#include "{hdr}"\n#include <stddef.h>\n'
           '_Static_assert(sizeof(fdgpu_precompile_t) == 12, "txn");\n'
           '_Static_assert(sizeof(fdgpu_precompile_info_t) == 16 && offsetof(fdgpu_precompile_info_t, ed_code) == 8, "info");\n'
           '_Static_assert(sizeof(fdgpu_precompile_walk_t) == 16 && offsetof(fdgpu_precompile_walk_t, code) == 12, "walk");\n'
           'int main(void){ fdgpu_precompile_t s; (void)s; return FDGPU_CODE_PRECOMPILE_DATA_SIZE + 70 + '
           'FDGPU_CODE_PRECOMPILE_DATA_OFFSET + 71 + FDGPU_CODE_PRECOMPILE_SIGNATURE + 72 + FDGPU_CODE_PRECOMPILE_CAP + 73; }\n')
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-x", "c", "-", "-fsyntax-only"], input=src,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    code = re.sub(r"/\*.*?\*/", "", open(hdr).read(), flags=re.S)
    assert set(re.findall(r"#include\s*[<\"]([^>\"]+)", code)) <= {"stddef.h", "stdint.h", "fd_ed25519_gpu.h"}
    assert "secp256k1" in open(hdr).read()                      # the header says what it skips
    names = _lib.header_functions(hdr)
    assert names == ["fdgpu_debug_precompile_time", "fdgpu_debug_precompile_walk", "fdgpu_poll_precompiles",
                     "fdgpu_precompile_sig_bound", "fdgpu_submit_precompiles"]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for n in names:
        assert re.search(r"\sT\s" + n + r"$", out, flags=re.M), n
    tout = subprocess.run(["nm", "-D", "--defined-only", tile.TILE_LIB_PATH], capture_output=True, text=True,
                          check=True).stdout
    for n in ("fdt_precompile_walk", "fdt_precompile_verdict", "fdgpu_precompiles_verify", "fdgpu_block_precompile_verify"):
        assert re.search(r"\sT\s" + n + r"$", tout, flags=re.M), n
    from firedancer_amd import ed25519 as ed
    assert ed.PRECOMPILE_DTYPE.itemsize == 12 and ed.PRECOMPILE_INFO_DTYPE.itemsize == 16
    assert ed.PRECOMPILE_WALK_DTYPE.itemsize == 16 and tile.PRECOMPILE_REC_DTYPE.itemsize == 12
    assert (ed.CODE_PRECOMPILE_DATA_SIZE, ed.CODE_PRECOMPILE_DATA_OFFSET, ed.CODE_PRECOMPILE_SIGNATURE,
            ed.CODE_PRECOMPILE_CAP) == (-70, -71, -72, -73)


def test_sanitizer_program(tmp_path, cases):
    """tools/precompile_san.cpp under ASan + UBSan: the parse, the walk and
    the verdict over the case set and 100,000 mutated payloads, each buffer in
    an allocation of its exact size."""
    exe = tmp_path / "precompile_san"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", "-I", os.path.join(REPO, "include"),
                        os.path.join(REPO, "tools", "precompile_san.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:          # [u32 size][i8 structural code or -64][u16 records][bytes] per case
        for c in cases:
            if c.model is None:
                code, n = PF, 0
            else:
                code, _, _, _, recs = pp.walk(*c.model)
                n = len(recs)
            f.write(len(c.payload).to_bytes(4, "little") + int(code).to_bytes(1, "little", signed=True) +
                    n.to_bytes(2, "little") + c.payload)
    r = subprocess.run([str(exe), str(path), "100000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    m = re.search(r"cases (\d+) ok, random (\d+): (\d+) parsed, (\d+) records", r.stdout)
    assert m and int(m.group(1)) == len(cases) and int(m.group(2)) == 100000, r.stdout
    assert int(m.group(3)) > 20000 and int(m.group(4)) > 20000, r.stdout       # the mutations reach the walk
