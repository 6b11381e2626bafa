"""The shred checks and the Merkle root against the reference's own code (CPU
only): tests/golden/shred_reference.json records what its fd_shred_parse and
fd_fec_resolver_add_shred decided about every case of pyref_shred.corpus().
A first shred is accepted by the resolver only if the leader's signature
verifies over the root the resolver computed itself, so an accepted case
whose signature was made over pyref_shred's root proves the two roots equal."""
import os

import numpy as np
import pytest

import pyref_shred as ps
from conftest import GOLDEN, REPO, load_json
from firedancer_amd import tile, workload

VERSION = ps.CORPUS_VERSION
REF_LIB = os.path.join(REPO, "oracle", "_ref", "libshred_ref.so")


@pytest.fixture(scope="module")
def golden():
    return load_json("shred_reference.json")


@pytest.fixture(scope="module")
def cases(golden):
    return ps.judged_corpus(golden, workload.sign)


def test_python_reference_agrees_with_the_reference(cases):
    for i, c in enumerate(cases):
        chk = ps.check(c["buf"], VERSION)
        # the checks pass exactly when the parse succeeded and the resolver did not reject a sealed case; a case
        # changed after sealing in bytes the checks do not read passes them whatever the resolver said
        assert (chk is not None) == (c["want"] != "reject"), (i, c["family"])
        if c["accepted"]:
            root = ps.shred_root(c["buf"], VERSION)
            # the root the reference verified the signature over is the one this file computes
            assert root == ps.lenient_root(c["buf"]), (i, c["family"])
            assert workload.sign(ps.CORPUS_PRV, root)[1] == c["buf"][:64], (i, c["family"])


def test_host_library_agrees_with_the_reference(oracle, cases):
    for i, c in enumerate(cases):
        want = ps.check(c["buf"], VERSION)
        assert tile.shred_check(c["buf"], VERSION) == want, (i, c["family"])
        assert (want is not None) == (c["want"] != "reject"), (i, c["family"])
        assert tile.shred_root(c["buf"], VERSION) == ps.shred_root(c["buf"], VERSION), (i, c["family"])

    def fn(a, t):
        return [oracle.verify(bytes(a[int(x["msg_off"]):int(x["msg_off"]) + int(x["msg_sz"])]),
                              bytes(a[int(x["sig_off"]):int(x["sig_off"]) + 64]),
                              bytes(a[int(x["pub_off"]):int(x["pub_off"]) + 32])) for x in t]

    arena, recs = ps.pack([c["buf"] for c in cases], [workload.sign(ps.CORPUS_PRV, b"")[0]])
    codes, roots = tile.shreds_verify(tile.PyVerifier(fn), arena, recs, VERSION, batch_max=1000)
    for i, c in enumerate(cases):
        assert ps.code_as_wanted(int(codes[i]), c["want"]), (i, c["family"], int(codes[i]), c["want"])
        r = ps.shred_root(c["buf"], VERSION)
        assert roots[i].tobytes() == (r if r is not None else bytes(32)), (i, c["family"])
    # family 9's twins changed after sealing: the checks pass, the signature does not
    twins = [int(codes[i]) for i, c in enumerate(cases) if c["family"] == "09_protected_bytes" and c["kind"] == "tamper"]
    assert len(twins) >= 30 and all(t not in (0, ps.CODE_SHRED_REJECT) for t in twins)


@pytest.mark.skipif(not os.path.exists(REF_LIB), reason="oracle/_ref/libshred_ref.so is built only where the reference tree is")
def test_live_judge_equals_the_golden_file(golden, cases):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_shred_golden", os.path.join(GOLDEN, "make_shred_golden.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    parse, rv = mk.judge(cases, workload.sign(ps.CORPUS_PRV, b"")[0], VERSION, REF_LIB)
    assert parse == golden["parse"]
    assert rv == golden["resolver"]
    mk.guards([c["family"] for c in cases], [c["kind"] for c in cases], parse, rv)
    assert np.count_nonzero(np.array(rv) == 0) >= 500
