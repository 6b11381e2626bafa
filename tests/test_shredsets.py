"""Set batches on the host (CPU only): fdgpu_shred_sets_verify against the
Python model over the oracle, its argument errors, the new header's ABI, and
the sanitizer program."""
import os
import re
import subprocess

import numpy as np
import pytest

import pyref_shred as ps
import pyref_shredsets as pss
from conftest import REPO
from firedancer_amd import _lib, tile, workload

VERSION = 0x1234


def oracle_fn(oracle):
    def fn(a, t):
        return [oracle.verify(bytes(a[int(x["msg_off"]):int(x["msg_off"]) + int(x["msg_sz"])]),
                              bytes(a[int(x["sig_off"]):int(x["sig_off"]) + 64]),
                              bytes(a[int(x["pub_off"]):int(x["pub_off"]) + 32])) for x in t]
    return fn


@pytest.fixture(scope="module")
def mixed():
    shreds, key_of, keys, _ = pss.mixed(VERSION, np.random.default_rng(31), workload.sign)
    return pss.pack(shreds, keys, key_of)


@pytest.fixture(scope="module")
def known():
    return pss.known_mix(VERSION, np.random.default_rng(32), workload.sign)


def test_whole_sets_cost_one_verify_each(oracle, mixed):
    arena, recs = mixed
    assert len(recs) == 110
    want_codes, want_roots, groups = pss.model(arena, recs, VERSION, oracle.verify)
    assert len(groups) == len(pss.MIXED_SETS) and (want_codes == 0).all()
    ver = tile.PyVerifier(oracle_fn(oracle))
    codes, roots, rep, lanes = tile.shred_sets_verify(ver, arena, recs, VERSION, batch_max=2)
    assert codes.tolist() == want_codes.tolist() and (roots == want_roots).all()
    assert pss.check_reps(rep, lanes, groups, len(recs)) == lanes == len(pss.MIXED_SETS) < len(recs)
    assert sum(ver.batches) == lanes and max(ver.batches) <= 2          # the verifier saw one item per set
    assert all(int(rep[i]) == idx[0] for idx in groups.values() for i in idx)   # the host's choice: a group's first shred
    # the same codes and roots as one verify per shred
    c1, r1 = tile.shreds_verify(tile.PyVerifier(oracle_fn(oracle)), arena, pss.drop_known(recs), VERSION)
    assert c1.tolist() == codes.tolist() and (r1 == roots).all()


def test_known_roots_and_rejects(oracle, known):
    arena, recs = known
    want_codes, want_roots, groups = pss.model(arena, recs, VERSION, oracle.verify)
    vals = want_codes.tolist()
    assert vals.count(pss.CODE_SHRED_ROOT_MISMATCH) >= 8 and vals.count(pss.CODE_SHRED_REJECT) == 6
    assert (recs["known_off"] != pss.NO_ROOT).sum() >= 40 and vals.count(0) >= 90
    ver = tile.PyVerifier(oracle_fn(oracle))
    codes, roots, rep, lanes = tile.shred_sets_verify(ver, arena, recs, VERSION)
    assert codes.tolist() == vals and (roots == want_roots).all()
    assert pss.check_reps(rep, lanes, groups, len(recs)) == lanes
    # a mismatch still reports the derived root, a rejected shred zeros whatever it names as known
    mism = np.flatnonzero(want_codes == pss.CODE_SHRED_ROOT_MISMATCH)
    assert roots[mism].any(axis=1).all()
    assert not roots[want_codes == pss.CODE_SHRED_REJECT].any()
    # every shred with a known root, and every shred rejected: no verify at all
    allk = recs.copy()
    allk["known_off"] = np.where(allk["known_off"] == pss.NO_ROOT, recs["known_off"][0], allk["known_off"])
    ver2 = tile.PyVerifier(oracle_fn(oracle))
    c2, r2, rep2, lanes2 = tile.shred_sets_verify(ver2, arena, allk, VERSION)
    w2, wr2, g2 = pss.model(arena, allk, VERSION, oracle.verify)
    assert lanes2 == 0 and not g2 and not ver2.batches and (rep2 == pss.NO_REP).all()
    assert c2.tolist() == w2.tolist() and (r2 == wr2).all()
    rej = recs[want_codes == pss.CODE_SHRED_REJECT]
    c3, r3, rep3, lanes3 = tile.shred_sets_verify(ver2, arena, rej, VERSION)
    assert lanes3 == 0 and not ver2.batches and (c3 == pss.CODE_SHRED_REJECT).all() and not r3.any()


def test_same_signature_different_keys(oracle, mixed):
    """A flipped payload byte gives a shred its own root, a wrong leader its
    own key: each is a group of its own and fails alone; a shred sent twice is
    one key."""
    arena, recs = mixed
    arena = arena.copy()
    a, b, c = 5, 17, 40
    arena[int(recs["off"][a]) + 200] ^= 0x40
    recs = np.concatenate([recs, recs[c:c + 1]])
    other = sorted(set(recs["pub_off"].tolist()) - {int(recs["pub_off"][b])})[0]
    recs["pub_off"][b] = other
    want_codes, want_roots, groups = pss.model(arena, recs, VERSION, oracle.verify)
    assert len(groups) == len(pss.MIXED_SETS) + 2
    assert want_codes[a] != 0 and want_codes[b] != 0 and (np.delete(want_codes, [a, b]) == 0).all()
    codes, roots, rep, lanes = tile.shred_sets_verify(tile.PyVerifier(oracle_fn(oracle)), arena, recs, VERSION)
    assert codes.tolist() == want_codes.tolist() and (roots == want_roots).all()
    assert pss.check_reps(rep, lanes, groups, len(recs)) == lanes
    assert rep[a] == a and rep[b] == b and rep[len(recs) - 1] == rep[c]


def test_argument_errors(oracle, mixed):
    arena, recs = mixed
    ver = tile.PyVerifier(oracle_fn(oracle))
    for field, val in (("known_off", len(arena) - 31), ("off", len(arena) - 100), ("pub_off", len(arena) - 31)):
        bad = recs[:8].copy()
        bad[field][3] = val
        with pytest.raises(RuntimeError):
            tile.shred_sets_verify(ver, arena, bad, VERSION)
    c, r, rep, lanes = tile.shred_sets_verify(ver, arena, recs[:0], VERSION)
    assert len(c) == 0 and lanes == 0


def test_shred_sets_header_abi():
    hdr = _lib.SHRED_SETS_HEADER_PATH
    src = (f'#include "{hdr}"\n_Static_assert(sizeof(fdgpu_set_shred_t) == 16, "set shred");\n'
           '_Static_assert(FDGPU_SHRED_NO_ROOT == 0xffffffffu, "no root");\n'
           'int main(void){ fdgpu_set_shred_t s; (void)s; return FDGPU_CODE_SHRED_ROOT_MISMATCH + 74; }\n')
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-x", "c", "-", "-fsyntax-only"], input=src,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    code = re.sub(r"/\*.*?\*/", "", open(hdr).read(), flags=re.S)
    assert set(re.findall(r"#include\s*[<\"]([^>\"]+)", code)) == {"stddef.h", "stdint.h", "fd_shred_gpu.h"}
    names = _lib.header_functions(hdr)
    assert names == ["fdgpu_debug_shred_sets_time", "fdgpu_poll_shred_sets", "fdgpu_submit_shred_sets"], names
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for n in names:
        assert re.search(r"\sT\s" + n + r"$", out, flags=re.M), n
    # the new code is no other header's
    inc = os.path.join(REPO, "include")
    vals = []
    for h in os.listdir(inc):
        vals += [int(v) for v in re.findall(r"#define\s+FDGPU_CODE_\w+\s+\((-\d+)\)", open(os.path.join(inc, h)).read())]
    assert vals.count(-74) == 1 and len(vals) == len(set(vals)), sorted(vals)
    from firedancer_amd import ed25519 as ed
    assert ed.SET_SHRED_DTYPE == tile.SET_SHRED_DTYPE == pss.SET_SHRED_DTYPE and ed.SET_SHRED_DTYPE.itemsize == 16
    assert ed.CODE_SHRED_ROOT_MISMATCH == tile.CODE_SHRED_ROOT_MISMATCH == pss.CODE_SHRED_ROOT_MISMATCH == -74
    assert ed.SHRED_NO_ROOT == tile.SHRED_NO_ROOT == pss.NO_ROOT
    tout = subprocess.run(["nm", "-D", "--defined-only", tile.TILE_LIB_PATH], capture_output=True, text=True,
                          check=True).stdout
    assert re.search(r"\sT\sfdgpu_shred_sets_verify$", tout, flags=re.M)
    assert "fdgpu_shred_sets_verify" in tile.header_functions()


def test_sanitizer_program(tmp_path, known):
    """tools/shred_sets_san.cpp under ASan + UBSan: the host rule and dedup
    over the known-root batch and 20,000 batches drawn from it, some with an
    offset at or past the arena's end, every buffer in an allocation of its
    exact size."""
    exe = tmp_path / "shred_sets_san"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", "-I", os.path.join(REPO, "include"),
                        os.path.join(REPO, "tools", "shred_sets_san.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    arena, recs = known
    codes, _, groups = pss.model(arena, recs, VERSION, lambda m, s, p: 0)
    rep = np.full(len(recs), pss.NO_REP, dtype="<u4")
    for idx in groups.values():
        rep[idx] = idx[0]
    batch = tmp_path / "batch.bin"
    with open(batch, "wb") as f:
        f.write(len(recs).to_bytes(4, "little") + len(arena).to_bytes(4, "little") + arena.tobytes() + recs.tobytes()
                + codes.tobytes() + rep.tobytes() + len(groups).to_bytes(4, "little"))
    r = subprocess.run([str(exe), str(batch), str(VERSION), "20000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    m = re.search(r"batch (\d+) ok, lanes (\d+), random (\d+): (\d+) ran, (\d+) refused", r.stdout)
    assert m and int(m.group(1)) == len(recs) and int(m.group(2)) == len(groups) and int(m.group(3)) == 20000, r.stdout
    assert int(m.group(4)) > 1000 and int(m.group(5)) > 1000, r.stdout
