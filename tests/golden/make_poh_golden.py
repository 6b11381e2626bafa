"""Writes tests/golden/poh_vectors.json: the two mainnet PoH vectors of the
reference's src/ballet/poh/test_poh.c:135-165 as data -- a pre hash, the steps
(append counts and mixins) and the post hash of each.  Reads the reference
tree (a sibling directory `reference`, or $FD_REFERENCE_TREE) when run; the
tests read only the file.

    python tests/golden/make_poh_golden.py
"""
import json
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "poh_vectors.json")
SRC = "src/ballet/poh/test_poh.c"


def hexbytes(text):
    return "".join(re.findall(r"_\((\w\w)\)", text))


def main():
    ref = os.environ.get("FD_REFERENCE_TREE") or os.path.join(os.path.dirname(REPO), "reference")
    text = open(os.path.join(ref, SRC)).read()
    steps = {}
    for name, body in re.findall(r"fd_poh_test_step_t const (\w+)\[\] = \{(.*?)\n\};", text, flags=re.S):
        out = []
        for item in re.findall(r"\{\s*\.(n\s*=\s*-?\d+|mixin\s*=\s*\{[^}]*\})\s*\}", body):
            if item.startswith("n"):
                n = int(item.split("=")[1])
                if n >= 0:
                    out.append({"append": n})
            else:
                out.append({"mixin": hexbytes(item)})
        steps[name] = out
    vectors = []
    for name, pre, post, st in re.findall(
            r"\.name\s*=\s*\"([^\"]+)\",\s*\.pre\s*=\s*\{([^}]*)\},\s*\.post\s*=\s*\{([^}]*)\},\s*\.steps\s*=\s*(\w+)", text):
        vectors.append({"name": name, "pre": hexbytes(pre), "steps": steps[st], "post": hexbytes(post)})
    assert len(vectors) == 2 and all(len(v["pre"]) == 64 and len(v["post"]) == 64 for v in vectors), vectors
    assert [len(v["steps"]) for v in vectors] == [1, 7]
    with open(OUT, "w") as f:
        json.dump({"source": SRC + ":135-165 (https://github.com/solana-foundation/specs/blob/main/core/poh.md)",
                   "vectors": vectors}, f, indent=1)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
