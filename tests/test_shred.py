"""The shred path on the host (CPU only): the Python reference against the
golden bmtree vectors, the host library's SHA-256, checks and Merkle root
against the Python reference, fdgpu_shreds_verify over the oracle, the new
header's ABI, and the sanitizer program."""
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import pyref_shred as ps
from conftest import GOLDEN, REPO, load_json
from firedancer_amd import _lib, tile, workload

VERSION = 0x1234
PRV = bytes(range(1, 33))


@pytest.fixture(scope="module")
def matrix():
    return ps.matrix(PRV, VERSION, np.random.default_rng(11), workload.sign)


@pytest.fixture(scope="module")
def rejects():
    return ps.reject_cases(PRV, VERSION, np.random.default_rng(12), workload.sign)


def test_python_builder_matches_golden():
    v = load_json("bmtree_vectors.json")
    leaves = [ps.hash_leaf(s.encode(), v["tree32"]["prefix_sz"]) for s in v["tree32"]["leaves"]]
    assert len(leaves) == 11
    root, _, _ = ps.bmtree(leaves, 32, 1)
    assert root.hex() == v["tree32"]["root"]
    for n, want in v["tree20"]["roots"].items():
        root, _, _ = ps.bmtree([i.to_bytes(8, "little") + bytes(12) for i in range(int(n))], 20, 1)
        assert root[:20].hex() == want, n
    gold = open(os.path.join(GOLDEN, v["proofs"]["file"]), "rb").read()
    assert len(gold) == 880
    root, _, proofs = ps.bmtree(leaves, 20, 1)
    for i in range(11):
        assert b"".join(proofs[i]) == gold[80 * i:80 * i + 80], i
        # and the proof walks back to the root (the rule fdt_shred_root applies, here with 1-byte prefixes)
        cur = leaves[i]
        for layer, node in enumerate(proofs[i]):
            pair = node + cur[:20] if (i >> layer) & 1 else cur[:20] + node
            cur = hashlib.sha256(ps.NODE_PREFIX[:1] + pair).digest()
        assert cur == root, i


def test_fec_set_proofs_walk_to_the_signed_root():
    shreds, root = ps.fec_set(5, 6, ps.T_DATA_CH, ps.T_CODE_CH, PRV, VERSION, np.random.default_rng(3), workload.sign)
    for s in shreds:
        assert ps.shred_root(s, VERSION) == root


def test_host_sha256_matches_hashlib():
    rng = np.random.default_rng(5)
    blob = rng.integers(0, 256, 1300, dtype=np.uint8).tobytes()
    for n in list(range(0, 201)) + list(range(1100, 1261)):
        assert tile.sha256(blob[:n]) == hashlib.sha256(blob[:n]).digest(), n


def test_shred_root_matrix(matrix):
    assert len(matrix) > 200
    mods = set()
    for b, root in matrix:
        chk = tile.shred_check(b, VERSION)
        want = ps.check(b, VERSION)
        assert chk == want, (hex(b[0x40]), want)
        assert tile.shred_root(b, VERSION) == root
        mods.add((26 + chk["leaf_end"] - chk["leaf_off"]) % 64)
    assert {57, 61, 62} <= mods, mods                  # the padding spills into an extra block
    assert any(m < 56 for m in mods), mods             # and the usual case
    assert {b[0x40] & 0xF0 for b, _ in matrix} == set(ps.TYPES)
    assert {b[0x40] & 0xF for b, _ in matrix} == set(range(10))


REJECT_NAMES = ["sz_87", "data_sz_1202", "code_sz_1227", "variant_a5", "variant_5a", "type_30", "zero_sig",
                "wrong_version", "data_cnt_0", "data_cnt_68", "code_cnt_0", "code_cnt_68", "code_idx_67",
                "idx_below_fec_set_idx", "depth_10", "depth_15", "idx4_depth2", "data_size_overflow"]


def test_every_reject_rule(rejects):
    assert set(rejects) == set(REJECT_NAMES) | {"idx3_depth2_ok"}
    for name in REJECT_NAMES:
        assert ps.check(rejects[name], VERSION) is None, name
        assert tile.shred_check(rejects[name], VERSION) is None, name
        assert tile.shred_root(rejects[name], VERSION) is None, name
    ok = rejects["idx3_depth2_ok"]
    assert tile.shred_check(ok, VERSION) == ps.check(ok, VERSION) and ps.check(ok, VERSION)["shred_idx"] == 3
    assert len(rejects["sz_87"]) == 87 and len(rejects["data_sz_1202"]) == 1202 and len(rejects["code_sz_1227"]) == 1227
    assert rejects["zero_sig"][:64] == bytes(64)


def test_mutations_agree_with_python(matrix):
    rng = np.random.default_rng(77)
    accepted = dropped = 0
    for k in range(200):
        b = bytearray(matrix[int(rng.integers(0, len(matrix)))][0])
        pos = int(rng.integers(0x40, 0x5A)) if k % 2 else int(rng.integers(0, len(b)))   # half in the header fields
        b[pos] ^= 1 << int(rng.integers(0, 8))
        want = ps.shred_root(b, VERSION)
        assert tile.shred_root(b, VERSION) == want, (k, pos)
        accepted += want is not None
        dropped += want is None
    assert accepted >= 20 and dropped >= 20, (accepted, dropped)


@pytest.fixture(scope="module")
def batch(oracle):
    return ps.verify_batch(VERSION, np.random.default_rng(21), workload.sign, oracle.verify)


def test_shreds_verify_over_the_oracle(oracle, batch):
    arena, recs, want_codes, want_roots = batch
    assert 380 <= len(recs) <= 430
    vals = want_codes.tolist()
    assert vals.count(0) >= 200
    for c in (-1, -2, -3, ps.CODE_SHRED_REJECT):
        assert c in vals, c

    def fn(a, t):
        return [oracle.verify(bytes(a[int(x["msg_off"]):int(x["msg_off"]) + int(x["msg_sz"])]),
                              bytes(a[int(x["sig_off"]):int(x["sig_off"]) + 64]),
                              bytes(a[int(x["pub_off"]):int(x["pub_off"]) + 32])) for x in t]

    ver = tile.PyVerifier(fn)
    codes, roots = tile.shreds_verify(ver, arena, recs, VERSION, batch_max=100)
    assert codes.tolist() == vals
    assert (roots == want_roots).all()
    assert len(ver.batches) >= 3 and max(ver.batches) <= 100
    bad = recs.copy()
    bad["off"][5] = len(arena)
    with pytest.raises(RuntimeError):
        tile.shreds_verify(ver, arena, bad, VERSION)


def test_shred_header_abi():
    hdr = _lib.SHRED_HEADER_PATH
    src = (f'#include "{hdr}"\n_Static_assert(sizeof(fdgpu_shred_t) == 12, "shred");\n'
           'int main(void){ fdgpu_shred_t s; (void)s; return FDGPU_CODE_SHRED_REJECT + 67; }\n')
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-x", "c", "-", "-fsyntax-only"], input=src,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    code = re.sub(r"/\*.*?\*/", "", open(hdr).read(), flags=re.S)
    assert set(re.findall(r"#include\s*[<\"]([^>\"]+)", code)) == {"stddef.h", "stdint.h", "fd_ed25519_gpu.h"}
    names = _lib.header_functions(hdr)
    assert names == sorted(["fdgpu_submit_shreds", "fdgpu_poll_shreds", "fdgpu_debug_sha256",
                            "fdgpu_debug_shred_roots", "fdgpu_debug_shred_time"]), names
    out = subprocess.run(["nm", "-D", "-C", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    syms = [ln.split(None, 2)[2] for ln in out.splitlines() if len(ln.split(None, 2)) == 3]
    for n in names:
        assert n in syms, n
    assert not [s for s in syms if "fdgpu::" in s]
    from firedancer_amd import ed25519 as ed
    assert ed.SHRED_DTYPE.itemsize == tile.SHRED_DTYPE.itemsize == 12 and ed.CODE_SHRED_REJECT == -67
    tout = subprocess.run(["nm", "-D", "--defined-only", tile.TILE_LIB_PATH], capture_output=True, text=True,
                          check=True).stdout
    for n in ("fdt_shred_check", "fdt_shred_root", "fdt_sha256", "fdgpu_shreds_verify"):
        assert re.search(r"\sT\s" + n + r"$", tout, flags=re.M), n


def test_sanitizer_program(tmp_path, rejects, matrix):
    """tools/shred_san.cpp under ASan + UBSan: the checks and the root over
    the reject cases and 100,000 random and mutated buffers, each in an
    allocation of its exact size."""
    exe = tmp_path / "shred_san"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", "-I", os.path.join(REPO, "include"),
                        os.path.join(REPO, "tools", "shred_san.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    cases = tmp_path / "cases.bin"
    with open(cases, "wb") as f:                 # [u32 size][u8 expected: 1 pass / 0 drop][bytes] per case
        for name, b in rejects.items():
            f.write(len(b).to_bytes(4, "little") + bytes([ps.check(b, VERSION) is not None]) + bytes(b))
        for b, _ in matrix[::7]:
            f.write(len(b).to_bytes(4, "little") + b"\x01" + bytes(b))
    r = subprocess.run([str(exe), str(cases), str(VERSION), "100000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    m = re.search(r"cases (\d+) ok, random (\d+): (\d+) passed the checks", r.stdout)
    assert m and int(m.group(1)) == len(rejects) + len(matrix[::7]) and int(m.group(2)) == 100000, r.stdout
    assert int(m.group(3)) > 1000, r.stdout              # the mutated ones keep reaching the hash
