"""Python model of a set batch (include/fd_shred_sets_gpu.h): every shred of a
batch to its code and root, one verify per distinct (signature, root, leader
key), shreds with a known root held against it.  Stated over pyref_shred's
checks and root and any verify(msg, sig, pub); the builders pack shreds, keys
and known roots into one arena."""
import numpy as np

import pyref_shred as ps

CODE_SHRED_REJECT = ps.CODE_SHRED_REJECT
CODE_SHRED_ROOT_MISMATCH = -74
NO_ROOT = 0xFFFFFFFF
NO_REP = 0xFFFFFFFF
SET_SHRED_DTYPE = np.dtype([("off", "<u4"), ("sz", "<u4"), ("pub_off", "<u4"), ("known_off", "<u4")])


def model(arena, recs, version, verify):
    """-> (codes int8[n], roots uint8[n, 32], groups: key bytes -> the indices
    of the shreds that carry it, in order).  verify runs once per key."""
    raw = bytes(arena)
    n = len(recs)
    codes = np.zeros(n, dtype=np.int8)
    roots = np.zeros((n, 32), dtype=np.uint8)
    groups = {}
    for i, r in enumerate(recs):
        off, sz, pub_off, known_off = (int(r[k]) for k in ("off", "sz", "pub_off", "known_off"))
        root = ps.shred_root(raw[off:off + sz], version)
        if root is None:
            codes[i] = CODE_SHRED_REJECT
            continue
        roots[i] = np.frombuffer(root, dtype=np.uint8)
        if known_off != NO_ROOT:
            codes[i] = 0 if raw[known_off:known_off + 32] == root else CODE_SHRED_ROOT_MISMATCH
            continue
        groups.setdefault(raw[off:off + 64] + root + raw[pub_off:pub_off + 32], []).append(i)
    for key, idx in groups.items():
        codes[idx] = verify(key[64:96], key[:64], key[96:])
    return codes, roots, groups


def pack(shreds, keys, key_of=None, known=None):
    """pyref_shred.pack with the known roots behind the keys: known[i] is None
    or the 32 bytes shred i's set is trusted to have -> (arena, SET_SHRED_DTYPE
    records)"""
    arena, r3 = ps.pack(shreds, keys, key_of)
    recs = np.zeros(len(r3), dtype=SET_SHRED_DTYPE)
    for k in ("off", "sz", "pub_off"):
        recs[k] = r3[k]
    recs["known_off"] = NO_ROOT
    blob, at = bytearray(), {}
    for i, kr in enumerate(known or []):
        if kr is None:
            continue
        kr = bytes(kr)
        if kr not in at:
            at[kr] = len(arena) + len(blob)
            blob += kr
        recs["known_off"][i] = at[kr]
    return np.concatenate([arena, np.frombuffer(bytes(blob), dtype=np.uint8)]), recs


def drop_known(recs):
    """the records as fdgpu_submit_shreds takes them"""
    out = np.zeros(len(recs), dtype=np.dtype([("off", "<u4"), ("sz", "<u4"), ("pub_off", "<u4")]))
    for k in ("off", "sz", "pub_off"):
        out[k] = recs[k]
    return out


def check_reps(rep, lanes, groups, n):
    """What every implementation owes beside the codes: rep[i] lies in i's own
    group and is its own representative, a shred outside every group has none,
    and lanes counts the representatives.  -> the number of distinct keys"""
    member = {}
    for g, idx in enumerate(groups.values()):
        for i in idx:
            member[i] = g
    assert len(rep) == n
    for i in range(n):
        if i in member:
            r = int(rep[i])
            assert r in member and member[r] == member[i], (i, r)
            assert int(rep[r]) == r, (i, r)
        else:
            assert int(rep[i]) == NO_REP, i
    assert lanes == len({int(rep[i]) for i in member})
    return len(groups)


MIXED_SETS = ((1, 1, ps.T_DATA, ps.T_CODE, 0), (2, 2, ps.T_DATA_CH, ps.T_CODE_CH, 1), (5, 3, ps.T_DATA, ps.T_CODE, 1),
              (32, 32, ps.T_DATA_CH, ps.T_CODE_CH, 0), (16, 16, ps.T_DATA, ps.T_CODE, 1))
PRVS = (bytes(range(1, 33)), bytes(range(2, 34)))


def mixed(version, rng, sign):
    """Whole FEC sets 1:1, 2:2, 5:3, 32:32 and 16:16 -- data and code, chained
    and plain, under two leaders -- interleaved and shuffled: 110 shreds
    -> (list of bytearray, key_of, keys, the sets' roots per shred)"""
    keys = [sign(p, b"")[0] for p in PRVS]
    shreds, key_of, roots = [], [], []
    for k, (dc, cc, td, tc, who) in enumerate(MIXED_SETS):
        s, root = ps.fec_set(dc, cc, td, tc, PRVS[who], version, rng, sign, fec_set_idx=100 * k)
        shreds += s
        key_of += [who] * len(s)
        roots += [root[:32]] * len(s)
    order = rng.permutation(len(shreds))
    return [shreds[i] for i in order], [key_of[i] for i in order], keys, [roots[i] for i in order]


def known_mix(version, rng, sign):
    """mixed() and six shreds the checks drop; of every three shreds one with
    its set's root as the known one, of every seven one with a wrong known
    root, the rest without -> (arena, records)"""
    shreds, key_of, keys, roots = mixed(version, rng, sign)
    rej = list(ps.reject_cases(PRVS[0], version, rng, sign).values())[:6]
    known = [r if i % 3 == 0 else bytes(32) if i % 7 == 0 else None for i, r in enumerate(roots)]
    known += [roots[0], None, bytes(32), None, roots[1], None]
    return pack(shreds + [bytearray(b) for b in rej], keys, key_of + [0] * 6, known)


def stream(version, rng, sign, n):
    """n shreds cut from a stream of 32:32 sets in order, so that a set spans
    each boundary at a multiple of 64 (a wave, a dedup workgroup)
    -> (shreds, key_of, keys)"""
    keys = [sign(PRVS[0], b"")[0]]
    shreds = []
    k = 0
    shreds += ps.fec_set(16, 16, ps.T_DATA, ps.T_CODE, PRVS[0], version, rng, sign, fec_set_idx=7)[0]   # shifts the sets by 32
    while len(shreds) < n:
        k += 1
        shreds += ps.fec_set(32, 32, ps.T_DATA, ps.T_CODE, PRVS[0], version, rng, sign, fec_set_idx=100 * k)[0]
    return shreds[:n], [0] * n, keys
