"""Writes tests/golden/shred_reference.json: what the reference's own
fd_shred_parse and fd_fec_resolver_add_shred decide about every case of
pyref_shred.corpus(), through oracle/_ref/libshred_ref.so (built by
`make -C oracle ref REF=<reference tree>`, which __graft_entry__.build() runs
where the tree is present).  The file holds the verdicts and the corpus's
SHA-256, not the shreds: the tests regenerate those from the committed seed.

    python tests/golden/make_shred_golden.py
"""
import collections
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import pyref_shred as ps  # noqa: E402
from firedancer_amd import workload  # noqa: E402

LIB = os.path.join(REPO, "oracle", "_ref", "libshred_ref.so")
OUT = os.path.join(HERE, "shred_reference.json")


def judge(cases, pub, version, path=LIB):
    """-> (parse results, resolver return values) of the reference for the cases"""
    lib = ctypes.CDLL(path)
    lib.shred_ref_parse.argtypes = [ctypes.c_char_p, ctypes.c_ulong]
    lib.shred_ref_add.argtypes = [ctypes.c_char_p, ctypes.c_ulong, ctypes.c_char_p, ctypes.c_ushort]
    parse = [int(lib.shred_ref_parse(c["buf"], len(c["buf"]))) for c in cases]
    rv = [int(lib.shred_ref_add(c["buf"], len(c["buf"]), pub, version)) for c in cases]
    return parse, rv


def guards(families, kinds, parse, rv):
    """The floors the corpus has to keep (asserted here and again by the tests) -> per-family [accepted, rejected]"""
    acc = [ps.ref_accepts(p, r) for p, r in zip(parse, rv)]
    assert all(r in (0, ps.REF_REJECTED, ps.REF_NO_PARSE) for r in rv), sorted(set(rv))   # never IGNORED or COMPLETES
    assert all((r == ps.REF_NO_PARSE) == (not p) for p, r in zip(parse, rv))
    assert sum(acc) >= 500 and len(acc) - sum(acc) >= 500, (sum(acc), len(acc) - sum(acc))
    per = collections.OrderedDict()
    for f, a in zip(families, acc):
        per.setdefault(f, [0, 0])[0 if a else 1] += 1
    for f, (a, r) in per.items():
        if f[:2] not in ("04", "07"):
            assert a and r, (f, a, r)
    assert len(per) == 10, list(per)
    return per


def main():
    cases = ps.corpus(workload.sign)
    pub = workload.sign(ps.CORPUS_PRV, b"")[0]
    parse, rv = judge(cases, pub, ps.CORPUS_VERSION)
    families = [c["family"] for c in cases]
    kinds = [c["kind"] for c in cases]
    per = guards(families, kinds, parse, rv)
    names = sorted(set(families))
    doc = {
        "comment": "verdicts of the reference's fd_shred_parse and fd_fec_resolver_add_shred (fresh resolver per case) "
                   "over pyref_shred.corpus(); written by make_shred_golden.py",
        "seed": ps.CORPUS_SEED,
        "version": ps.CORPUS_VERSION,
        "sha256": ps.corpus_digest(cases),
        "n": len(cases),
        "families": names,
        "family": [names.index(f) for f in families],
        "tamper": [int(k == "tamper") for k in kinds],
        "sz": [len(c["buf"]) for c in cases],
        "parse": parse,
        "resolver": rv,
    }
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"{OUT}: {len(cases)} cases, sha256 {doc['sha256']}")
    print(f"{'family':<22}{'accepted':>9}{'rejected':>9}")
    for fam, (a, r) in per.items():
        print(f"{fam:<22}{a:>9}{r:>9}")
    print(f"{'total':<22}{sum(a for a, _ in per.values()):>9}{sum(r for _, r in per.values()):>9}")
    mism = [i for i, c in enumerate(cases)
            if c["kind"] == "checks" and (ps.check(c["buf"], ps.CORPUS_VERSION) is not None) != ps.ref_accepts(parse[i], rv[i])]
    print(f"cases where pyref_shred.check disagrees with the reference: {len(mism)}")
    for i in mism[:40]:
        b = cases[i]["buf"]
        print(f"  #{i} {families[i]} sz {len(b)} variant {b[0x40]:#04x} parse {parse[i]} resolver {rv[i]}")


if __name__ == "__main__":
    main()
