"""A hashlib model of the PoH check (include/fd_poh_gpu.h): what
fd_runtime_poh_verify_wide_task computes per entry -- fd_poh_append, the
32-byte / 1-byte-prefix Merkle root of the entry's signatures
(fd_wbmtree32), fd_poh_mixin -- an evaluator of a whole batch as the engine
takes it, and a generator of batches for the tests."""
import hashlib

import numpy as np

from firedancer_amd.ed25519 import CODE_POH_MISMATCH, CODE_POH_TOO_LONG, POH_DTYPE, POH_NO_MIX


def sha256(b):
    return hashlib.sha256(b).digest()


def append(h, n):
    """fd_poh_append"""
    h = bytes(h)
    for _ in range(int(n)):
        h = sha256(h)
    return h


def mixin(h, m):
    """fd_poh_mixin"""
    return sha256(bytes(h) + bytes(m))


def leaf(data):
    return sha256(b"\x00" + bytes(data))


def fold(nodes):
    """The root over given leaf hashes: a branch is SHA-256(0x01 || l || r), a
    layer's odd last node is paired with itself, one leaf is its own root."""
    nodes = [bytes(x) for x in nodes]
    assert nodes
    while len(nodes) > 1:
        if len(nodes) & 1:
            nodes.append(nodes[-1])
        nodes = [sha256(b"\x01" + nodes[i] + nodes[i + 1]) for i in range(0, len(nodes), 2)]
    return nodes[0]


def sig_root(sigs):
    return fold([leaf(s) for s in sigs])


def entry_hash(prev, hash_cnt, sigs=(), mix=None):
    """out of one entry: sigs its 64-byte signatures, or mix 32 bytes mixed in as given"""
    assert not (sigs and mix is not None)
    if not sigs and mix is None:
        return append(prev, hash_cnt)
    h = append(prev, hash_cnt - 1 if hash_cnt else 0)
    return mixin(h, sig_root(sigs) if sigs else mix)


def evaluate(arena, entries, sig_offs, cap):
    """A batch as fdgpu_submit_poh takes it -> (codes int8[n], hashes uint8[n, 32])"""
    raw = bytes(np.asarray(arena, dtype=np.uint8))
    codes = np.zeros(len(entries), dtype=np.int8)
    hashes = np.zeros((len(entries), 32), dtype=np.uint8)
    for i, e in enumerate(entries):
        hc = int(e["hash_cnt"])
        if hc > cap:
            codes[i] = CODE_POH_TOO_LONG
            continue
        first, cnt, mo = int(e["sig_first"]), int(e["sig_cnt"]), int(e["mix_off"])
        sigs = [raw[int(o):int(o) + 64] for o in sig_offs[first:first + cnt]]
        mix = raw[mo:mo + 32] if mo != POH_NO_MIX else None
        out = entry_hash(raw[int(e["prev_off"]):int(e["prev_off"]) + 32], hc, sigs, mix)
        hashes[i] = np.frombuffer(out, dtype=np.uint8)
        if out != raw[int(e["hash_off"]):int(e["hash_off"]) + 32]:
            codes[i] = CODE_POH_MISMATCH
    return codes, hashes


class Batch:
    """Builds a batch whose every entry claims its true hash.  Signature j of
    the batch sits at arena alignment j mod 16; prev and claimed hashes sit at
    odd offsets.  corrupt() then spoils single entries."""

    def __init__(self, rng):
        self.rng = rng
        self.arena = bytearray(rng.integers(0, 256, 7, dtype=np.uint8).tobytes())
        self.entries, self.sig_offs = [], []

    def _put(self, data, mod, of):
        while len(self.arena) % of != mod:
            self.arena.append(int(self.rng.integers(0, 256)))
        off = len(self.arena)
        self.arena += data
        return off

    def _rand(self, n):
        return self.rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    def add(self, hash_cnt, n_sig=0, mix=False, prev=None):
        """an entry of hash_cnt hashes: a tick, or with n_sig signatures, or with a given mix"""
        prev = self._rand(32) if prev is None else bytes(prev)
        sigs = [self._rand(64) for _ in range(n_sig)]
        m = self._rand(32) if mix else None
        out = entry_hash(prev, hash_cnt, sigs, m)
        first = len(self.sig_offs)
        for s in sigs:
            self.sig_offs.append(self._put(s, len(self.sig_offs) % 16, 16))
        self.entries.append((hash_cnt, self._put(prev, 1, 2), self._put(out, 1, 2), first, n_sig,
                             self._put(m, len(self.entries) % 4, 4) if mix else POH_NO_MIX, 0))
        return out

    def arrays(self):
        """-> (arena uint8[], entries POH_DTYPE[], sig_offs uint32[])"""
        return (np.frombuffer(bytes(self.arena), dtype=np.uint8).copy(), np.array(self.entries, dtype=POH_DTYPE),
                np.array(self.sig_offs, dtype=np.uint32))


def corrupt(arena, entries, sig_offs, i, how, rng):
    """Spoils entry i in place: one bit of its claimed hash ("hash"), of one of
    its signatures ("sig"), of its prev hash ("prev"), or hash_cnt +-1
    ("cnt+", "cnt-")."""
    e = entries[i]
    bit = 1 << int(rng.integers(0, 8))
    if how == "hash":
        arena[int(e["hash_off"]) + int(rng.integers(0, 32))] ^= bit
    elif how == "prev":
        arena[int(e["prev_off"]) + int(rng.integers(0, 32))] ^= bit
    elif how == "sig":
        assert e["sig_cnt"]
        j = int(e["sig_first"]) + int(rng.integers(0, int(e["sig_cnt"])))
        arena[int(sig_offs[j]) + int(rng.integers(0, 64))] ^= bit
    elif how == "cnt+":
        entries["hash_cnt"][i] += 1
    elif how == "cnt-":
        assert e["hash_cnt"] > 1
        entries["hash_cnt"][i] -= 1
    else:
        raise ValueError(how)


SIG_CNTS = (1, 2, 3, 4, 5, 7, 8, 9, 11, 31, 32, 33, 63, 64, 65, 127, 129)


def matrix(chunk, rng):
    """hash_cnt in {0, 1, 2, 3, CHUNK-1, CHUNK, CHUNK+1, 2 CHUNK+1} x {a tick,
    an entry with a mix, an entry with each of SIG_CNTS signatures} -> Batch"""
    b = Batch(rng)
    for hc in (0, 1, 2, 3, chunk - 1, chunk, chunk + 1, 2 * chunk + 1):
        b.add(hc)
        b.add(hc, mix=True)
        for ns in SIG_CNTS:
            b.add(hc, n_sig=ns)
    return b


def mixed(n, rng, lo=1, hi=5000):
    """n entries of lengths lo..hi: a third ticks, a third mixes, a third with 1..4 signatures"""
    b = Batch(rng)
    for i in range(n):
        hc = int(rng.integers(lo, hi + 1))
        kind = i % 3
        b.add(hc, n_sig=int(rng.integers(1, 5)) if kind == 2 else 0, mix=kind == 1)
    return b


def golden_entries(vec):
    """A golden vector (pre, steps, post) as a chained Batch: an append of n
    followed by a mixin is one entry of n + 1 hashes carrying that mix, a
    lone append a tick.  -> (Batch, the last entry's claimed hash)"""
    b = Batch(np.random.default_rng(1))
    h = bytes.fromhex(vec["pre"])
    steps = vec["steps"]
    k = 0
    while k < len(steps):
        n = steps[k]["append"]
        if k + 1 < len(steps) and "mixin" in steps[k + 1]:
            m = bytes.fromhex(steps[k + 1]["mixin"])
            out = mixin(append(h, n), m)
            mo = b._put(m, 1, 2)
            b.entries.append((n + 1, b._put(h, 1, 2), b._put(out, 1, 2), 0, 0, mo, 0))
            k += 2
        else:
            out = append(h, n)
            b.entries.append((n, b._put(h, 1, 2), b._put(out, 1, 2), 0, 0, POH_NO_MIX, 0))
            k += 1
        h = out
    return b, h


def stream(rng, payloads, sigs_of, blocks=3, per_block=8, hi=300):
    """The entries of `blocks` blocks in order, chained from in_hash through
    their claimed hashes: every other entry carries 1..3 of the raw
    transactions `payloads` (sigs_of(payload) -> its signatures), the rest are
    ticks.  -> dict(in_hash, hash_cnt, entry_hash, txn_cnt, payloads)"""
    pool = list(payloads)
    in_hash = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
    s = {"in_hash": in_hash, "hash_cnt": [], "entry_hash": [], "txn_cnt": [], "payloads": []}
    h = in_hash
    for i in range(blocks * per_block):
        hc = int(rng.integers(1, hi + 1))
        txs = [pool.pop() for _ in range(int(rng.integers(1, 4)))] if i % 2 == 0 and i % per_block != per_block - 1 else []
        h = entry_hash(h, hc, [x for p in txs for x in sigs_of(p)])
        s["hash_cnt"].append(hc)
        s["entry_hash"].append(h)
        s["txn_cnt"].append(len(txs))
        s["payloads"] += txs
    return s
