"""Python reference for the shred path, written with hashlib: the checks the
shred tile makes before the signature, the Merkle root from a shred's
inclusion proof, a binary Merkle tree builder, and generators of shreds and
FEC sets.

The tree builder is pinned to the reference implementation by the golden
vectors (tests/golden/bmtree_vectors.json, bmtree_reference_proofs.bin);
everything else in the shred tests is pinned to this file.

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
