"""Python-integer models of the layer between the field and the verify chain:
the radix-2^25.5 limb vectors of csrc/fdgpu_fe.h and their bound classes, the
signed fixed-window recodings of csrc/fdgpu_sc.h, the points the group-op test
runs (csrc/fdgpu_ge.h) and the fixed-base comb table (csrc/fdgpu_bcomb.h).

TEST INFRASTRUCTURE ONLY.  Everything here is exact integer arithmetic on top
of pyref_ed25519 (textbook addition); nothing restates a kernel's formula.
"""
import hashlib
import json

import numpy as np

import pyref_ed25519 as ref
from pyref_ed25519 import D, L, P

# ------------------------------------------------------------------ limbs
WIDTH = [26 if i % 2 == 0 else 25 for i in range(10)]
POS = [25 * i + (i + 1) // 2 for i in range(10)]          # weight of limb i: 2^(25 i + ceil(i/2))
assert POS == [0, 26, 51, 77, 102, 128, 153, 179, 204, 230]


def limbs_value(limbs):
    """The residue a limb vector stands for (any non-negative limbs)."""
    return sum(int(v) << POS[i] for i, v in enumerate(limbs)) % P


def limbs_of(x):
    """The canonical limb vector of an integer 0 <= x < 2^255."""
    return [(x >> POS[i]) & ((1 << WIDTH[i]) - 1) for i in range(10)]


def limbs_of_kp(k):
    """k * p with every limb k times p's (how FDGPU_FE_2P / _4P are written)."""
    return [k * v for v in limbs_of(P)]


P2 = limbs_of_kp(2)
P4 = limbs_of_kp(4)

# The bound classes of the table at the head of fdgpu_fe.h, as that table
# states them: one maximum for every limb, R with its slack on limbs 1 and 5.
R15_SLACK = 150562                                         # floor(2^17.2)
CLASS_MAX = {"R": [1 << 26] * 10, "A": [1 << 27] * 10, "S": [(1 << 26) + (1 << 27)] * 10,
             "S4": [(1 << 26) + (1 << 28)] * 10}
CLASS_ORDER = ["R", "A", "S", "S4"]
# membership lets limbs 1 and 5 carry the slack the classes inherit from R
# (A = R + R twice it, S and S4 once)
_SLACK = {"R": 1, "A": 2, "S": 1, "S4": 1}
CLASS_LIMIT = {c: [m + (_SLACK[c] * R15_SLACK if i in (1, 5) else 0) for i, m in enumerate(CLASS_MAX[c])]
               for c in CLASS_ORDER}
R15_MAX = CLASS_LIMIT["R"]
# the operand-class pairs the header declares valid for fe_mul(first, second)
MUL_PAIRS = [("R", "R"), ("A", "A"), ("S", "S"), ("A", "S"), ("S", "A"), ("S4", "A")]


def class_of(limbs):
    """The smallest class whose limits cover the vector, or None."""
    for c in CLASS_ORDER:
        if all(int(v) <= m for v, m in zip(limbs, CLASS_LIMIT[c])):
            return c
    return None


def mul_in_contract(f, g):
    """fe_mul(f, g) as the header admits it: R, A, S for both operands; S4
    only first, with the second at most A."""
    cf, cg = class_of(f), class_of(g)
    if cf is None or cg is None:
        return False
    if cf == "S4":
        return cg in ("R", "A")
    return cg != "S4"


def mul_conditions(fmax, gmax):
    """The three conditions fe_mul's exactness rests on, for limb maxima."""
    return (267 * max(fmax) * max(gmax) < 1 << 64, all(2 * v < 1 << 32 for v in fmax),
            all(19 * v < 1 << 32 for v in gmax))


FE_RAW_OPS = ["mul", "sq", "add", "sub", "sub_mul", "neg", "neg_mul", "canon", "sub4", "sub4_mul"]


def fe_raw_expected(f, g):
    """Expected residues of debug_fe_raw's ten results for one record, None
    where the record is outside that operation's precondition:
      fe_mul    the header's operand classes (mul_in_contract)
      fe_sq     "inputs up to A/S"
      fe_add    sums that fe_tobytes takes (limbs <= 2^31)
      fe_sub    g <= R and no limb of 2p - g below zero; fe_sub4: g <= A, against 4p
      fe_neg    f <= R and no limb of 2p - f below zero
    and a product of a difference only where the difference's own limbs and g
    are an admitted pair."""
    f, g = [int(v) for v in f], [int(v) for v in g]
    vf, vg = limbs_value(f), limbs_value(g)
    cf, cg = class_of(f), class_of(g)
    out = dict.fromkeys(FE_RAW_OPS)
    if mul_in_contract(f, g):
        out["mul"] = vf * vg % P
    if cf in ("R", "A", "S"):
        out["sq"] = vf * vf % P
    if all(a + b <= 1 << 31 for a, b in zip(f, g)):
        out["add"] = (vf + vg) % P
    out["canon"] = vf
    if cg == "R" and all(b <= m for b, m in zip(g, P2)):
        d = [a + m - b for a, b, m in zip(f, g, P2)]
        out["sub"] = (vf - vg) % P
        if mul_in_contract(d, g):
            out["sub_mul"] = (vf - vg) * vg % P
    if cf == "R" and all(a <= m for a, m in zip(f, P2)):
        d = [m - a for a, m in zip(f, P2)]
        out["neg"] = -vf % P
        if mul_in_contract(d, g):
            out["neg_mul"] = -vf * vg % P
    if cg in ("R", "A") and all(b <= m for b, m in zip(g, P4)):
        d = [a + m - b for a, b, m in zip(f, g, P4)]
        out["sub4"] = (vf - vg) % P
        if mul_in_contract(d, g):
            out["sub4_mul"] = (vf - vg) * vg % P
    return out


def words_value(w):
    """8 little-endian u32 words -> integer."""
    return int.from_bytes(np.ascontiguousarray(w, dtype="<u4").tobytes(), "little")


def value_words(x):
    return np.frombuffer(int(x).to_bytes(32, "little"), dtype="<u4")


def canonical_limbs_to_ints(arr):
    """uint32[n, 10] canonical limbs (every limb below its width, so the bit
    fields do not overlap) -> list of n integers."""
    arr = np.ascontiguousarray(arr, dtype=np.uint32)
    words = np.zeros((len(arr), 4), dtype=np.uint64)
    for i, pos in enumerate(POS):
        w, sh = pos >> 6, pos & 63
        v = arr[:, i].astype(np.uint64)
        words[:, w] |= v << np.uint64(sh)
        if sh + WIDTH[i] > 64:
            words[:, w + 1] |= v >> np.uint64(64 - sh)
    b = words.astype("<u8").tobytes()
    return [int.from_bytes(b[32 * k:32 * k + 32], "little") for k in range(len(arr))]


def fe_raw_records(seed=0xFE2A, n_random=300):
    """The (f, g) limb records of the raw field-op test: for every operand
    pair the header admits (and R with its slack on limbs 1 and 5), all limbs
    at the class maximum, one limb at the maximum in each position against a
    full and against a lone partner, and n_random uniform vectors inside the
    classes; subtrahends drawn inside what fe_sub / fe_sub4 / fe_neg take;
    zero and the limb vectors of p, 2p, 4p; padded with uniform R vectors to
    64 k + 1 records."""
    import random
    rnd = random.Random(seed)
    pairs = [(CLASS_MAX[a], CLASS_MAX[b]) for a, b in MUL_PAIRS] + [(R15_MAX, R15_MAX)]
    uni = lambda mx: [rnd.randint(0, m) for m in mx]          # noqa: E731
    one = lambda mx, i: [m if k == i else 0 for k, m in enumerate(mx)]   # noqa: E731
    recs = []
    for fm, gm in pairs:
        recs.append((fm, gm))
        for i in range(10):
            recs += [(one(fm, i), gm), (fm, one(gm, i)), (one(fm, i), one(gm, (10 - i) % 10)), (one(fm, i), one(gm, i))]
        recs += [(uni(fm), uni(gm)) for _ in range(n_random)]
    zero, p1 = [0] * 10, limbs_of_kp(1)
    specials = [zero, p1, P2, P4]
    for f in specials:
        for g in specials[:3] + [CLASS_MAX["R"], CLASS_MAX["A"]]:
            recs.append((f, g))
    # differences feeding a product, as the point formulas form them: g inside what the subtraction takes
    sub_g = [min(a, b) for a, b in zip(R15_MAX, P2)]
    sub4_g = [min(a, b) for a, b in zip(CLASS_LIMIT["A"], P4)]
    for fm in (CLASS_MAX["R"], R15_MAX, CLASS_MAX["A"], sub_g):
        for gm in (sub_g, sub4_g):
            recs += [(fm, gm), (zero, gm), (fm, zero)]
            recs += [(uni(fm), uni(gm)) for _ in range(n_random // 2)]
    while len(recs) % 64 != 1:
        recs.append((uni(CLASS_MAX["R"]), uni(CLASS_MAX["R"])))
    return np.array([list(f) + list(g) for f, g in recs], dtype=np.uint32)


# -------------------------------------------------------------- recodings
def signed_digits(x, w, n):
    """The unique digits d_0..d_{n-1} in [-2^(w-1), 2^(w-1)) with
    x = sum d_i 2^(w i), or None when x has no such representation.  Adding
    2^(w-1) to every digit makes them the plain radix-2^w digits of
    x + sum 2^(w-1) 2^(w i)."""
    half = 1 << (w - 1)
    y = x + sum(half << (w * i) for i in range(n))
    if y >> (w * n):
        return None
    return [((y >> (w * i)) & ((1 << w) - 1)) - half for i in range(n)]


def unpack_digits(words, slot, n):
    """n two's-complement slots of `slot` bits from packed u32 words."""
    x = sum(int(v) << (32 * i) for i, v in enumerate(words))
    out = []
    for i in range(n):
        d = (x >> (slot * i)) & ((1 << slot) - 1)
        out.append(d - (1 << slot) if d >> (slot - 1) else d)
    return out


# ----------------------------------------------------------------- points
O = (0, 1, 1, 0)


def affine(pt):
    zi = ref._inv(pt[2])
    x, y = pt[0] * zi % P, pt[1] * zi % P
    return (x, y, 1, x * y % P)


def neg(pt):
    return (-pt[0] % P, pt[1], pt[2], -pt[3] % P)


def niels(pt):
    """(y+x, y-x, 2dxy) of a point's affine form."""
    x, y, _, _ = affine(pt)
    return ((y + x) % P, (y - x) % P, 2 * D * x * y % P)


def on_curve(pt):
    X, Y, Z, T = pt
    return (Z % P != 0 and (-X * X + Y * Y - Z * Z - D * T * T) % P == 0 and (T * Z - X * Y) % P == 0)


def torsion_points():
    """The eight points of order dividing 8, affine: O, (0, -1), the two of
    order 4 (+-sqrt(-1), 0) and the four of order 8."""
    from firedancer_amd.workload import SMALL_ORDER_ENC
    pts = [O, (0, P - 1, 1, 0), (ref.SQRTM1, 0, 1, 0), (P - ref.SQRTM1, 0, 1, 0)]
    pts += [ref.decode(bytes.fromhex(h)) for h in SMALL_ORDER_ENC[4:]]
    return pts


def rescale(pt, lam):
    return tuple(c * lam % P for c in pt)


# ------------------------------------------------------------- comb table
def comb_bases(w, ndig):
    """2^(w i) B for i < ndig, by w doublings each from the one before."""
    out, b = [], ref.B
    for _ in range(ndig):
        out.append(b)
        for _ in range(w):
            b = ref._add(b, b)
    return out


def table_points(base, entries):
    """j * base for j < entries, by repeated addition of the base."""
    pt = O
    for _ in range(entries):
        yield pt
        pt = ref._add(pt, base)


def entry_kind(j, chunk, entries):
    last = entries - 1
    if j == last:
        return "the table's last entry" + (", alone in its chunk" if last % chunk == 0 else "")
    if j % chunk == 0:
        return "a chunk's first entry"
    if j % chunk == chunk - 1:
        return "a chunk's last entry"
    return "inside a chunk"


def check_table(tab, w, chunk, select=None):
    """tab: uint32[ndig, entries, stride].  Every selected entry (select(i, j);
    None: all) must hold canonical limbs of values < p in words 0..29, zeros in
    words 30, 31, and the affine niels form of j 2^(w i) B, compared by
    cross-multiplication with the model's projective point.  Returns the first
    failure as text, or None."""
    ndig, entries, stride = tab.shape
    assert stride >= 32
    lim = np.array([1 << WIDTH[k % 10] for k in range(30)], dtype=np.uint32)
    for i, base in enumerate(comb_bases(w, ndig)):
        t = tab[i]
        bad = np.nonzero((t[:, :30] >= lim).any(axis=1) | (t[:, 30:] != 0).any(axis=1))[0]
        if select is not None:
            bad = [j for j in bad if select(i, int(j))]
        if len(bad):
            j = int(bad[0])
            return f"table {i} entry {j} ({entry_kind(j, chunk, entries)}): limbs not canonical or padding not zero"
        ypx, ymx, xy2d = (canonical_limbs_to_ints(t[:, 10 * c:10 * c + 10]) for c in range(3))
        for j, (X, Y, Z, _) in enumerate(table_points(base, entries)):
            if select is not None and not select(i, j):
                continue
            a, b, c = ypx[j], ymx[j], xy2d[j]
            if (a >= P or b >= P or c >= P or (a * Z - Y - X) % P or (b * Z - Y + X) % P
                    or (c * Z * Z - 2 * D * X * Y) % P):
                return f"table {i} entry {j} ({entry_kind(j, chunk, entries)}): not j * 2^({w} * {i}) B"
    return None


def subset_select(ndig, entries, chunk):
    """The entries checked where the whole table takes too long: tables 0 and
    ndig-1 whole; elsewhere entries 0..129, every chunk's first and last entry
    and the last 129."""
    def select(i, j):
        return (i in (0, ndig - 1) or j < 130 or j % chunk in (0, chunk - 1) or j >= entries - 129)
    return select


def model_table(w, ndig, entries, stride=32):
    """The table the model itself expects (one batch inversion per table)."""
    tab = np.zeros((ndig, entries, stride), dtype=np.uint32)
    for i, base in enumerate(comb_bases(w, ndig)):
        pts = list(table_points(base, entries))
        pre, acc = [], 1
        for pt in pts:
            pre.append(acc)
            acc = acc * pt[2] % P
        inv = ref._inv(acc)
        rows = [None] * entries
        for j in range(entries - 1, -1, -1):
            X, Y, Z, _ = pts[j]
            zi = inv * pre[j] % P
            inv = inv * Z % P
            x, y = X * zi % P, Y * zi % P
            rows[j] = limbs_of((y + x) % P) + limbs_of((y - x) % P) + limbs_of(2 * D * x * y % P)
        tab[i, :, :30] = np.array(rows, dtype=np.uint32)
    return tab


# ------------------------------------------------- comb edge signatures
def vectors_digest(vectors):
    return hashlib.sha256(json.dumps(vectors, sort_keys=True, separators=(",", ":")).encode()).hexdigest()


def hram(r_enc, pub, msg):
    return int.from_bytes(hashlib.sha512(r_enc + pub + msg).digest(), "little") % L


def encode(pt):
    x, y, _, _ = affine(pt)
    return (y | ((x & 1) << 255)).to_bytes(32, "little")
