"""Python reference for the shred path, written with hashlib: the checks the
shred tile makes before the signature, the Merkle root from a shred's
inclusion proof, a binary Merkle tree builder, and generators of shreds and
FEC sets.

The tree builder is pinned to the reference implementation by the golden
vectors (tests/golden/bmtree_vectors.json, bmtree_reference_proofs.bin); the
checks and the root are pinned to the reference's own parse and FEC resolver
by the verdicts recorded over corpus() (tests/golden/shred_reference.json);
the other shred tests are pinned to this file.

Shred layout (packed, little-endian): signature 0x00 (64 B), variant 0x40,
slot 0x41, idx 0x49, version 0x4d, fec_set_idx 0x4f; data shreds: parent_off
0x53, flags 0x55, size 0x56; code shreds: data_cnt 0x53, code_cnt 0x55, idx
0x57."""
import hashlib
import struct

import numpy as np

LEAF_PREFIX = b"\x00SOLANA_MERKLE_SHREDS_LEAF"
NODE_PREFIX = b"\x01SOLANA_MERKLE_SHREDS_NODE"
MIN_SZ, MAX_SZ = 1203, 1228
T_DATA, T_CODE, T_DATA_CH, T_CODE_CH, T_DATA_RS, T_CODE_RS = 0x80, 0x40, 0x90, 0x60, 0xB0, 0x70
TYPES = (T_DATA, T_CODE, T_DATA_CH, T_CODE_CH, T_DATA_RS, T_CODE_RS)
CODE_SHRED_REJECT = -67


def bmtree_depth(leaf_cnt):
    return leaf_cnt if leaf_cnt <= 1 else (leaf_cnt - 1).bit_length() + 1


def is_data(t):
    return (t & 0xC0) == 0x80


def chained(t):
    return t in (T_DATA_CH, T_CODE_CH, T_DATA_RS, T_CODE_RS)


def resigned(t):
    return t in (T_DATA_RS, T_CODE_RS)


def proof_off(t, depth):
    return (MIN_SZ if is_data(t) else MAX_SZ) - 20 * depth - 64 * resigned(t)


def check(buf, expected_version):
    """The parse and the pre-signature checks -> dict(shred_idx, depth,
    proof_off, leaf_off, leaf_end) or None."""
    buf = bytes(buf)
    sz = len(buf)
    if sz < 0x58:
        return None
    variant = buf[0x40]
    t = variant & 0xF0
    if t not in TYPES and variant not in (0xA5, 0x5A):
        return None
    legacy = t in (0xA0, 0x50)
    depth = 0 if legacy else variant & 0xF
    prev = 32 if chained(t) else 0
    if t & 0x80:
        size = struct.unpack_from("<H", buf, 0x56)[0]
        if size < 0x58:
            return None
        if t != 0xA0 and sz < MIN_SZ:
            return None
        effective = sz if t & 0x20 else MIN_SZ          # the resigned data type shares the legacy bit
        if effective < 0x58 + 20 * depth + (size - 0x58) + prev:
            return None
        need = effective
    elif t & 0x40:
        if 0x59 + prev + 20 * depth > MAX_SZ:
            return None
        need = MAX_SZ
    else:
        return None
    if sz < need:
        return None
    if buf[:64] == bytes(64):
        return None
    if legacy:
        return None
    if struct.unpack_from("<H", buf, 0x4D)[0] != expected_version:
        return None
    data_cnt = 0
    if not is_data(t):
        data_cnt, code_cnt = struct.unpack_from("<HH", buf, 0x53)
        if data_cnt > 67 or code_cnt > 67 or not data_cnt or not code_cnt:
            return None
        in_type_idx = struct.unpack_from("<H", buf, 0x57)[0]
    else:
        idx, fec = struct.unpack_from("<I", buf, 0x49)[0], struct.unpack_from("<I", buf, 0x4F)[0]
        in_type_idx = (idx - fec) & 0xFFFFFFFF
    if in_type_idx >= 67:
        return None
    shred_idx = in_type_idx if is_data(t) else in_type_idx + data_cnt
    if depth > 9:
        return None
    if bmtree_depth(shred_idx + 1) > depth + 1:
        return None
    po = proof_off(t, depth)
    return dict(shred_idx=shred_idx, depth=depth, proof_off=po, leaf_off=64, leaf_end=po)


def root_from(buf, chk):
    cur = hashlib.sha256(LEAF_PREFIX + bytes(buf[64:chk["proof_off"]])).digest()
    for layer in range(chk["depth"]):
        node = bytes(buf[chk["proof_off"] + 20 * layer: chk["proof_off"] + 20 * layer + 20])
        if (chk["shred_idx"] >> layer) & 1:
            cur = hashlib.sha256(NODE_PREFIX + node + cur[:20]).digest()
        else:
            cur = hashlib.sha256(NODE_PREFIX + cur[:20] + node).digest()
    return cur


def shred_root(buf, expected_version):
    chk = check(buf, expected_version)
    return None if chk is None else root_from(buf, chk)


def bmtree(leaves, hash_sz, prefix_sz):
    """Binary Merkle tree over leaf nodes (bytes, at least hash_sz each): a
    node is SHA-256(node_prefix[:prefix_sz] || left[:hash_sz] ||
    right[:hash_sz]); a layer's odd last node is merged with itself.
    -> (root: the top node, untruncated; layers; proofs: per leaf the
    hash_sz-byte siblings bottom-up)."""
    layers = [[bytes(x) for x in leaves]]
    while len(layers[-1]) > 1:
        cur, nxt = layers[-1], []
        for i in range(0, len(cur), 2):
            a, b = cur[i], cur[i + 1] if i + 1 < len(cur) else cur[i]
            nxt.append(hashlib.sha256(NODE_PREFIX[:prefix_sz] + a[:hash_sz] + b[:hash_sz]).digest())
        layers.append(nxt)
    proofs = []
    for i in range(len(leaves)):
        p, k = [], i
        for lay in layers[:-1]:
            sib = k ^ 1
            p.append((lay[sib] if sib < len(lay) else lay[k])[:hash_sz])
            k >>= 1
        proofs.append(p)
    return layers[-1][0], layers, proofs


def hash_leaf(data, prefix_sz):
    return hashlib.sha256(LEAF_PREFIX[:prefix_sz] + bytes(data)).digest()


# ------------------------------------------------------------- generators

def blank_shred(t, depth, rng, version, shred_idx=0, data_cnt=32, code_cnt=32, fec_set_idx=1000, slot=7):
    """A shred of type t (one of TYPES) with the given proof depth and leaf
    index, random payload and proof, signature zero (sign it with seal())."""
    sz = MIN_SZ if is_data(t) else MAX_SZ
    b = bytearray(rng.integers(0, 256, sz, dtype=np.uint8).tobytes())
    b[0:64] = bytes(64)
    b[0x40] = t | depth
    struct.pack_into("<Q", b, 0x41, slot)
    struct.pack_into("<H", b, 0x4D, version)
    struct.pack_into("<I", b, 0x4F, fec_set_idx)
    if is_data(t):
        struct.pack_into("<I", b, 0x49, (fec_set_idx + shred_idx) & 0xFFFFFFFF)
        cap = MIN_SZ - 0x58 - 20 * min(depth, 15) - (32 if chained(t) else 0) - (64 if resigned(t) else 0)
        struct.pack_into("<H", b, 0x56, 0x58 + max(0, min(cap, int(rng.integers(0, 900)))))
    else:
        cidx = shred_idx - data_cnt
        assert 0 <= cidx, "a code shred's leaf index is code.idx + data_cnt"
        struct.pack_into("<I", b, 0x49, fec_set_idx + cidx)
        struct.pack_into("<HHH", b, 0x53, data_cnt, code_cnt, cidx)
    return b


def seal(b, prv, version, sign):
    """Signs the shred's root (as the checks see it) into its first 64 bytes;
    a shred the checks drop gets a non-zero dummy signature.  -> root or None"""
    b[0:64] = b"\x01" * 64
    r = shred_root(b, version)
    if r is not None:
        b[0:64] = sign(prv, r)[1]
    return r


def fec_set(data_cnt, code_cnt, t_data, t_code, prv, version, rng, sign, fec_set_idx=64, slot=9):
    """A whole FEC set: data_cnt + code_cnt shreds whose proofs come from one
    tree (20-byte nodes, 26-byte prefixes), all carrying the leader's
    signature of its root.  -> (list of bytearray, root)"""
    n = data_cnt + code_cnt
    depth = bmtree_depth(n) - 1
    shreds = [blank_shred(t_data if i < data_cnt else t_code, depth, rng, version, i, data_cnt, code_cnt, fec_set_idx, slot)
              for i in range(n)]
    offs = [proof_off(t_data if i < data_cnt else t_code, depth) for i in range(n)]
    leaves = [hash_leaf(s[64:o], 26) for s, o in zip(shreds, offs)]
    root, _, proofs = bmtree(leaves, 20, 26)
    sig = sign(prv, root)[1]
    for s, o, p in zip(shreds, offs, proofs):
        s[o:o + 20 * depth] = b"".join(p)
        s[0:64] = sig
    return shreds, root


def pack(shreds, keys, key_of=None):
    """Shreds back to back (so every alignment occurs), the keys behind them.
    -> (arena uint8[], records with fields off, sz, pub_off)"""
    recs, blob = [], bytearray()
    for s in shreds:
        recs.append([len(blob), len(s), 0])
        blob += bytes(s)
    kbase = len(blob)
    for k in keys:
        blob += bytes(k)
    for i, r in enumerate(recs):
        r[2] = kbase + 32 * (key_of[i] if key_of is not None else 0)
    arr = np.zeros(len(recs), dtype=np.dtype([("off", "<u4"), ("sz", "<u4"), ("pub_off", "<u4")]))
    for i, r in enumerate(recs):
        arr[i] = tuple(r)
    return np.frombuffer(bytes(blob), dtype=np.uint8).copy(), arr


MATRIX_IDX = (0, 1, 2, 3, 66, 67, 85, 133)


def matrix(prv, version, rng, sign):
    """6 types x depth 0..9 x MATRIX_IDX, wherever the type and the depth
    rule admit the index -> list of (bytearray shred, root)"""
    out = []
    for t in TYPES:
        for depth in range(10):
            for idx in MATRIX_IDX:
                if bmtree_depth(idx + 1) > depth + 1:
                    continue
                if is_data(t):
                    if idx > 66:
                        continue
                    b = blank_shred(t, depth, rng, version, idx)
                else:
                    if idx < 1:
                        continue
                    dc = min(67, idx) if idx <= 67 else 67
                    if idx - dc > 66:
                        continue
                    b = blank_shred(t, depth, rng, version, idx, data_cnt=dc, code_cnt=67)
                r = seal(b, prv, version, sign)
                assert r is not None, (hex(t), depth, idx)
                out.append((b, r))
    return out


def reject_cases(prv, version, rng, sign):
    """One shred per reject rule -> dict name -> bytes (all dropped by check(),
    except the '_ok' companions)."""
    def data(depth=3, idx=2, t=T_DATA):
        return blank_shred(t, depth, rng, version, idx)

    def code(depth=7, idx=40, dc=32, cc=32, t=T_CODE):
        return blank_shred(t, depth, rng, version, idx, data_cnt=dc, code_cnt=cc)

    def sealed(b):
        seal(b, prv, version, sign)
        return bytes(b)

    c = {}
    c["sz_87"] = sealed(data())[:87]
    c["data_sz_1202"] = sealed(data())[:1202]
    c["code_sz_1227"] = sealed(code())[:1227]
    for v in (0xA5, 0x5A):
        b = data() if v == 0xA5 else code()
        b[0x40] = v
        c["variant_%02x" % v] = sealed(b)
    b = data(); b[0x40] = 0x30 | 3
    c["type_30"] = sealed(b)
    b = bytearray(sealed(data())); b[0:64] = bytes(64)
    c["zero_sig"] = bytes(b)
    b = data(); struct.pack_into("<H", b, 0x4D, (version + 1) & 0xFFFF)
    c["wrong_version"] = sealed(b)
    for name, off, val in (("data_cnt_0", 0x53, 0), ("data_cnt_68", 0x53, 68), ("code_cnt_0", 0x55, 0),
                           ("code_cnt_68", 0x55, 68), ("code_idx_67", 0x57, 67)):
        b = code(); struct.pack_into("<H", b, off, val)
        c[name] = sealed(b)
    b = data(); struct.pack_into("<I", b, 0x49, 999); struct.pack_into("<I", b, 0x4F, 1000)
    c["idx_below_fec_set_idx"] = sealed(b)
    for d in (10, 15):
        b = data(depth=9); b[0x40] = T_DATA | d
        struct.pack_into("<H", b, 0x56, 0x58)
        c["depth_%d" % d] = sealed(b)
    c["idx4_depth2"] = sealed(data(depth=2, idx=4))
    c["idx3_depth2_ok"] = sealed(data(depth=2, idx=3))
    b = data(depth=5); struct.pack_into("<H", b, 0x56, 0x58 + (MIN_SZ - 0x58 - 100) + 1)
    c["data_size_overflow"] = sealed(b)
    return c


_L = 2**252 + 27742317777372353535851937790883648493
SMALL_ORDER_KEY = bytes.fromhex("c7176a703d4dd84fba3c0b760d10670f2a2053fa2c39ccc64ec7fd7792ac037a")


def verify_batch(version, rng, sign, verify):
    """About 400 shreds from three FEC sets (32+32, 32+32, 67+67) with
    mutations (a flipped payload bit, proof byte, signature bit; S + L; a
    wrong and a small-order leader key) and the reject cases.  verify(msg,
    sig, pub) is the checker the expectation is built with.
    -> (arena, records, expected codes int8[], expected roots uint8[n, 32])"""
    prv, prv2 = bytes(range(1, 33)), bytes(range(2, 34))
    pub, pub2 = sign(prv, b"")[0], sign(prv2, b"")[0]
    keys = [pub, pub2, SMALL_ORDER_KEY]
    shreds, key_of = [], []
    for k, (dc, cc, td, tc) in enumerate(((32, 32, T_DATA, T_CODE), (32, 32, T_DATA_CH, T_CODE_CH),
                                          (67, 67, T_DATA_RS, T_CODE_RS))):
        s, _ = fec_set(dc, cc, td, tc, prv, version, rng, sign, fec_set_idx=100 * k)
        shreds += s
    key_of = [0] * len(shreds)
    n0 = len(shreds)
    for j in range(0, n0, 2):                    # every other shred once more, mutated
        b = bytearray(shreds[j])
        m = (j // 2) % 6
        po = check(b, version)["proof_off"]
        ko = 0
        if m == 0:
            b[64 + int(rng.integers(0, po - 64))] ^= 1 << int(rng.integers(0, 8))
            struct.pack_into("<H", b, 0x4D, version)         # (a flip in the version would be a reject: keep it a hash change)
        elif m == 1:
            if check(b, version)["depth"]:
                b[po + int(rng.integers(0, 20 * check(b, version)["depth"]))] ^= 0x10
        elif m == 2:
            b[int(rng.integers(0, 64))] ^= 1 << int(rng.integers(0, 8))
        elif m == 3:
            s_int = int.from_bytes(b[32:64], "little") + _L
            if s_int < 2**256:
                b[32:64] = s_int.to_bytes(32, "little")
        elif m == 4:
            ko = 1
        else:
            ko = 2
        shreds.append(b)
        key_of.append(ko)
    for name, b in reject_cases(prv, version, rng, sign).items():
        shreds.append(bytearray(b))
        key_of.append(0)
    arena, recs = pack(shreds, keys, key_of)
    codes = np.zeros(len(shreds), dtype=np.int8)
    roots = np.zeros((len(shreds), 32), dtype=np.uint8)
    for i, b in enumerate(shreds):
        r = shred_root(b, version)
        if r is None:
            codes[i] = CODE_SHRED_REJECT
        else:
            roots[i] = np.frombuffer(r, dtype=np.uint8)
            codes[i] = verify(r, bytes(b[:64]), keys[key_of[i]])
    return arena, recs, codes, roots


# ------------------------------------------------- the reference-judged corpus
#
# corpus() builds about 2,500 shreds aimed at the edges of the checks.  What the
# reference's own fd_shred_parse and fd_fec_resolver_add_shred decide about each
# is recorded in tests/golden/shred_reference.json (written by
# tests/golden/make_shred_golden.py through oracle/_ref/libshred_ref.so); the
# tests regenerate the corpus from CORPUS_SEED and compare this file, the host
# library and the GPU with those records.

CORPUS_SEED = "firedancer_amd shred reference corpus v1"
CORPUS_VERSION = 0x1234
CORPUS_PRV = bytes(range(1, 33))
REF_REJECTED, REF_NO_PARSE = -2, -100      # FD_FEC_RESOLVER_SHRED_REJECTED; the harness's "parse failed"


class CounterRng:
    """SHA-256 in counter mode over a seed string, with the integers(...)
    subset of numpy's Generator that this file uses: the bytes drawn do not
    depend on numpy's version."""

    def __init__(self, seed):
        self.seed, self.ctr, self.buf = seed.encode(), 0, b""

    def raw(self, n):
        while len(self.buf) < n:
            self.buf += hashlib.sha256(self.seed + self.ctr.to_bytes(8, "little")).digest()
            self.ctr += 1
        out, self.buf = self.buf[:n], self.buf[n:]
        return out

    def integers(self, low, high=None, size=None, dtype=None):
        if high is None:
            low, high = 0, low
        if size is None:
            return low + int.from_bytes(self.raw(8), "little") % (high - low)
        if (low, high) == (0, 256):
            return np.frombuffer(self.raw(size), dtype=np.uint8)
        return np.array([self.integers(low, high) for _ in range(size)], dtype=dtype)


def lenient_root(buf):
    """The root as the header fields alone give it, with no range checks:
    type, depth, proof offset and leaf index straight from the buffer; None
    where the type is neither data nor code or the leaf or proof would leave
    the buffer."""
    buf = bytes(buf)
    if len(buf) < 0x59:
        return None
    t, depth = buf[0x40] & 0xF0, buf[0x40] & 0xF
    if (t & 0xC0) == 0x80:
        end = MIN_SZ
        idx = (struct.unpack_from("<I", buf, 0x49)[0] - struct.unpack_from("<I", buf, 0x4F)[0]) & 0xFFFFFFFF
    elif (t & 0xC0) == 0x40:
        end = MAX_SZ
        idx = struct.unpack_from("<H", buf, 0x57)[0] + struct.unpack_from("<H", buf, 0x53)[0]
    else:
        return None
    end -= 64 if t in (T_DATA_RS, T_CODE_RS) else 0
    po = end - 20 * depth
    if end > len(buf) or po < 64:
        return None
    return root_from(buf, dict(shred_idx=idx, depth=depth, proof_off=po))


def seal_lenient(b, prv, sign):
    """The leader's signature over lenient_root(b), or a non-zero dummy where
    there is none: whatever the checks decide, the signature is not what
    drops the shred."""
    b[0:64] = b"\x01" * 64
    r = lenient_root(b)
    if r is not None:
        b[0:64] = sign(prv, r)[1]
    return r


CORPUS_IDX = (0, 1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 63, 64, 66, 67, 127, 128, 133)
CORPUS_SIZES = (87, 88, 89, 1202, 1203, 1204, 1227, 1228, 1229, 1232)


def _any_shred(t, depth, rng, version, idx, **kw):
    """blank_shred for any leaf index: a code shred takes data_cnt = min(67,
    idx) but at least 2 (a lone code shred with data_cnt 1 would complete its
    set in the reference and go on to Reed-Solomon, which is not the subject);
    None where a code shred cannot carry the index."""
    if is_data(t):
        return blank_shred(t, depth, rng, version, idx, **kw)
    dc = max(2, min(67, idx))
    if idx < dc:
        return None
    return blank_shred(t, depth, rng, version, idx, data_cnt=dc, code_cnt=67, **kw)


def corpus(sign):
    """-> list of dict(family, kind, buf): kind 'checks' is a shred sealed
    after its mutation (the reference drops it exactly if its checks do),
    kind 'tamper' one changed after sealing in bytes the checks do not read
    (the reference drops it exactly if the change reaches the root)."""
    rng, prv, ver = CounterRng(CORPUS_SEED), CORPUS_PRV, CORPUS_VERSION
    out = []

    def add(family, b, kind="checks", reseal=True):
        b = bytearray(b)
        if reseal:
            seal_lenient(b, prv, sign)
        t = b[0x40] & 0xF0 if len(b) > 0x54 else 0
        assert not ((t & 0xC0) == 0x40 and struct.unpack_from("<H", b, 0x53)[0] == 1), family
        out.append(dict(family=family, kind=kind, buf=bytes(b)))

    def resized(b, sz):
        return bytearray(b[:sz]) + bytearray(rng.integers(0, 256, max(0, sz - len(b)), dtype=np.uint8).tobytes())

    def flip(b, pos, bit=None):
        b = bytearray(b)
        b[pos] ^= 1 << (int(rng.integers(0, 8)) if bit is None else bit)
        return b

    # 1. the matrix, with the indices the depth rule or the type does not admit kept in
    good = []
    for t in TYPES:
        for depth in range(10):
            for idx in MATRIX_IDX:
                b = _any_shred(t, depth, rng, ver, idx)
                if b is None:
                    continue
                add("01_matrix", b)
                if check(out[-1]["buf"], ver) is not None:
                    good.append(out[-1]["buf"])
    # 2. packet sizes around every bound, the longer ones with random trailing bytes
    for t in TYPES:
        for depth in (0, 5, 9):
            for sz in CORPUS_SIZES:
                add("02_size", resized(_any_shred(t, depth, rng, ver, 0 if is_data(t) else 2), sz))
    # 3. data.size around the bound for either reading of the effective size
    for t in (T_DATA, T_DATA_CH, T_DATA_RS):
        for sz in (1203, 1228, 1232):
            for depth in (0, 7):
                sizes = {0, 0x57, 0x58, 0xFFFF}
                for eff in (MIN_SZ, sz):
                    bound = eff - 20 * depth - (32 if chained(t) else 0)
                    sizes |= {bound - 1, bound, bound + 1}
                for size in sorted(sizes):
                    b = resized(blank_shred(t, depth, rng, ver, 0), sz)
                    struct.pack_into("<H", b, 0x56, size)
                    add("03_data_size", b)
    # 4. every variant byte, on a data-sized and on a code-sized buffer
    for base in (blank_shred(T_DATA, 0, rng, ver, 2), blank_shred(T_CODE, 0, rng, ver, 34, data_cnt=32, code_cnt=32)):
        if len(base) == MIN_SZ:
            struct.pack_into("<H", base, 0x56, 0x58 + 100)
        for v in range(256):
            b = bytearray(base)
            b[0x40] = v
            add("04_variant", b)
    # 5. the count and index limits
    for t in (T_CODE, T_CODE_CH, T_CODE_RS):
        for off, vals in ((0x53, (0, 2, 67, 68, 0xFFFF)), (0x55, (0, 2, 67, 68, 0xFFFF)), (0x57, (0, 66, 67, 0xFFFF))):
            for val in vals:
                b = blank_shred(t, 9, rng, ver, 32, data_cnt=32, code_cnt=32)
                struct.pack_into("<H", b, off, val)
                add("05_limits", b)
        b = blank_shred(t, 9, rng, ver, 133, data_cnt=67, code_cnt=67)
        add("05_limits", b)
    for t in (T_DATA, T_DATA_CH, T_DATA_RS):
        for fec in (1000, 0, 0xFFFFFFC0, 0xFFFFFFFF):
            for d in (-1, 0, 66, 67):
                b = blank_shred(t, 9, rng, ver, 0, fec_set_idx=fec)
                struct.pack_into("<I", b, 0x49, (fec + d) & 0xFFFFFFFF)
                add("05_limits", b)
    # 6. the depth rule at every index where the minimal depth changes, and the depths past 9
    for t in TYPES:
        for idx in CORPUS_IDX:
            minimal = bmtree_depth(idx + 1) - 1
            for depth in (minimal - 1, minimal, minimal + 1, 10, 15):
                if depth < 0:
                    continue
                b = _any_shred(t, min(depth, 9), rng, ver, idx)
                if b is None:
                    continue
                b[0x40] = t | depth
                if is_data(t):
                    struct.pack_into("<H", b, 0x56, 0x58 + int(rng.integers(0, 400)))
                add("06_depth", b)
    # 7. the signature and the version
    for t, idx in ((T_DATA, 3), (T_CODE_CH, 40)):
        base = _any_shred(t, 6, rng, ver, idx)
        seal_lenient(base, prv, sign)
        assert check(base, ver) is not None
        z = bytearray(base); z[0:64] = bytes(64)
        add("07_signature", z, reseal=False)
        for pos in (0, 31, 32, 63):
            z = bytearray(base); z[0:64] = bytes(64); z[pos] = 1 + int(rng.integers(0, 255))
            add("07_signature", z, kind="tamper", reseal=False)
        for v in ((ver + 1) & 0xFFFF, (ver - 1) & 0xFFFF, ((ver & 0xFF) << 8) | (ver >> 8)):
            b = bytearray(base)
            struct.pack_into("<H", b, 0x4D, v)
            add("07_signature", b)
    # 8. bytes that must not matter, changed after sealing -- and next to each the last byte that does
    for t in TYPES:
        for depth in ((0, 4) if is_data(t) else (2, 4)):      # a code shred's least index is 2, its least depth too
            for sz in (1203, 1228, 1232):
                full = MIN_SZ if is_data(t) else MAX_SZ
                if sz < full:
                    continue
                base = resized(_any_shred(t, depth, rng, ver, 0 if is_data(t) else 2), sz)
                seal_lenient(base, prv, sign)
                assert check(base, ver) is not None
                inside_end = full - (64 if resigned(t) else 0)        # leaf, then proof, end here
                free = [p for p in (inside_end, inside_end + 63 if resigned(t) else None, full, sz - 1)
                        if p is not None and inside_end <= p < sz]
                for p in sorted(set(free)):
                    add("08_ignored_bytes", flip(base, p), kind="tamper", reseal=False)
                add("08_ignored_bytes", flip(base, inside_end - 1), kind="tamper", reseal=False)
    # 9. bytes that must matter: changed before sealing (accepted), and the same change after it
    for t in TYPES:
        depth = 3
        base = _any_shred(t, depth, rng, ver, 5)
        po = proof_off(t, depth)
        spots = [int(rng.integers(0x59, po - 32)), 0x41 + int(rng.integers(0, 8))] + [po + 20 * k + int(rng.integers(0, 20)) for k in range(depth)]
        if chained(t):
            spots.append(po - 32 + int(rng.integers(0, 32)))
        sealed = bytearray(base)
        seal_lenient(sealed, prv, sign)
        assert check(sealed, ver) is not None
        for p in spots:
            bit = int(rng.integers(0, 8))
            add("09_protected_bytes", flip(base, p, bit))
            add("09_protected_bytes", flip(sealed, p, bit), kind="tamper", reseal=False)
    # 10. random single-bit changes of accepted matrix shreds, half of them in the header fields, sealed again
    k = 0
    while k < 500:
        b = bytearray(good[int(rng.integers(0, len(good)))])
        pos = int(rng.integers(0x40, 0x5A)) if k % 2 else int(rng.integers(64, len(b)))
        b = flip(b, pos)
        if (b[0x40] & 0xC0) == 0x40 and struct.unpack_from("<H", b, 0x53)[0] == 1:
            continue                                   # data_cnt 1: see _any_shred
        add("10_random_bit", b)
        k += 1
    return out


def corpus_arena(cases):
    """The corpus as one byte string, each case behind its 2-byte length: the
    golden file pins the SHA-256 of these bytes."""
    return b"".join(len(c["buf"]).to_bytes(2, "little") + c["buf"] for c in cases)


def corpus_digest(cases):
    return hashlib.sha256(corpus_arena(cases)).hexdigest()


def ref_accepts(parse, rv):
    """the reference's verdict from its recorded parse result and resolver return value"""
    return bool(parse) and rv not in (REF_REJECTED, REF_NO_PARSE)


def judged_corpus(golden, sign):
    """corpus() checked against the golden file's SHA-256 and floors, each
    case with the reference's recorded verdict: `accepted`, and `want`, the
    code every implementation here owes it -- 'ok' (0) exactly where the
    reference accepted, 'reject' (CODE_SHRED_REJECT) exactly where it dropped
    a case of kind 'checks', 'sig' (a non-zero Ed25519 code) where it dropped
    one of kind 'tamper'."""
    cases = corpus(sign)
    assert golden["seed"] == CORPUS_SEED and golden["version"] == CORPUS_VERSION
    assert corpus_digest(cases) == golden["sha256"], "the regenerated corpus is not the one the reference judged"
    assert len(cases) == golden["n"] == len(golden["parse"]) == len(golden["resolver"]) == len(golden["family"])
    per = {}
    for c, f, tam, sz, p, rv in zip(cases, golden["family"], golden["tamper"], golden["sz"], golden["parse"],
                                    golden["resolver"]):
        assert c["family"] == golden["families"][f] and (c["kind"] == "tamper") == bool(tam) and len(c["buf"]) == sz
        assert rv in (0, REF_REJECTED, REF_NO_PARSE) and (rv == REF_NO_PARSE) == (not p)
        c["accepted"] = ref_accepts(p, rv)
        c["want"] = "ok" if c["accepted"] else "reject" if c["kind"] == "checks" else "sig"
        per.setdefault(c["family"], [0, 0])[0 if c["accepted"] else 1] += 1
    acc = sum(a for a, _ in per.values())
    assert acc >= 500 and len(cases) - acc >= 500, per
    assert len(per) == 10 and all(a and r for f, (a, r) in per.items() if f[:2] not in ("04", "07")), per
    return cases


def code_as_wanted(code, want):
    return code == 0 if want == "ok" else code == CODE_SHRED_REJECT if want == "reject" else code not in (0, CODE_SHRED_REJECT)
