"""Python mirror of the reference's Ed25519 verify interface, served by the
MI355X engine through the C ABI (include/fd_ed25519_gpu.h).

Reference interface (src/ballet/ed25519/fd_ed25519.h):
  FD_ED25519_SUCCESS / ERR_SIG / ERR_PUBKEY / ERR_MSG       :11-14
  fd_ed25519_verify(msg, msg_sz, sig, public_key, sha)      :96-101
  fd_ed25519_verify_batch_single_msg(msg, msg_sz, signatures, pubkeys, shas, batch_sz)  :124-130
  fd_ed25519_strerror(err)                                  :132-136

Same names (without the fd_ed25519_ prefix), argument meaning and codes;
the SHA-512 scratch objects are accepted and ignored (hashing is on the GPU).
The batched engine (VerifyEngine) is the throughput path used by the verify
stage; per-transaction results equal fd_ed25519_verify_batch_single_msg.
"""
import ctypes

import numpy as np

from . import _lib

SUCCESS, ERR_SIG, ERR_PUBKEY, ERR_MSG = 0, -1, -2, -3

FLAG_REF_MAPPING = 1
FLAG_NO_BUCKET = 2      # verify in transaction order instead of grouped by SHA-512 block count
FLAG_FULL_PATH = 4      # diagnostics: every signature through the full-length fallback kernel
FLAG_KEY_CACHE = 8      # one A decode + table per distinct public key of a batch (signer reuse)
FLAG_PAIR = 16          # two lanes per signature: a shorter verify for batches that leave the GPU idle
FLAG_PAIR_AUTO = 32     # the two-lane kernel for small ring batches while the engine is otherwise idle
FLAG_MERGE = 64         # gathered batches' verifies merged into shared launches
FLAG_SPREAD = 128       # one verify block per CU
FLAG_SPREAD_AUTO = 256  # ... while the engine's batches fit the chip that way

# fdgpu_txn_t as a numpy record (msg_off, msg_sz, sig_off, pub_off, sig_cnt)
TXN_DTYPE = np.dtype([("msg_off", "<u4"), ("msg_sz", "<u4"), ("sig_off", "<u4"),
                      ("pub_off", "<u4"), ("sig_cnt", "<u4")])
SIG_DESC_DTYPE = np.dtype([("msg_off", "<u4"), ("msg_sz", "<u4"), ("sig_off", "<u4"), ("pub_off", "<u4")])
TXN_DESC_DTYPE = np.dtype([("sig0", "<u4"), ("sig_cnt", "<u4")])
# the kernels' flags debug_verify_prehashed passes (csrc/fdgpu_internal.h: FDGPU_FLAG_REF_MAP, _KFULL, _KPAIR)
KFLAG_REF_MAP, KFLAG_FULL, KFLAG_PAIR = 1, 2, 8
ARENA_SLACK = 160
SHRED_DTYPE = np.dtype([("off", "<u4"), ("sz", "<u4"), ("pub_off", "<u4")])   # fdgpu_shred_t
CODE_SHRED_REJECT = -67       # FDGPU_CODE_SHRED_REJECT
SHRED_SZ_MAX = 1228 + 4       # FDGPU_SHRED_SZ_MAX
# fdgpu_set_shred_t (include/fd_shred_sets_gpu.h)
SET_SHRED_DTYPE = np.dtype([("off", "<u4"), ("sz", "<u4"), ("pub_off", "<u4"), ("known_off", "<u4")])
SHRED_NO_ROOT = 0xFFFFFFFF    # FDGPU_SHRED_NO_ROOT
CODE_SHRED_ROOT_MISMATCH = -74    # FDGPU_CODE_SHRED_ROOT_MISMATCH
# fdgpu_poh_entry_t (include/fd_poh_gpu.h)
POH_DTYPE = np.dtype([("hash_cnt", "<u8"), ("prev_off", "<u4"), ("hash_off", "<u4"), ("sig_first", "<u4"),
                      ("sig_cnt", "<u4"), ("mix_off", "<u4"), ("_pad", "<u4")])
POH_NO_MIX = 0xFFFFFFFF       # FDGPU_POH_NO_MIX
POH_HASH_CNT_MAX = 1 << 20    # FDGPU_POH_HASH_CNT_MAX
CODE_POH_MISMATCH = -68       # FDGPU_CODE_POH_MISMATCH
CODE_POH_TOO_LONG = -69       # FDGPU_CODE_POH_TOO_LONG
# include/fd_precompile_gpu.h
PRECOMPILE_DTYPE = np.dtype([("off", "<u4"), ("sz", "<u4"), ("sig_cap", "<u4")])   # fdgpu_precompile_t
PRECOMPILE_INFO_DTYPE = np.dtype([("instr_idx", "<u2"), ("rec_idx", "<u2"), ("ed_instr_cnt", "<u2"), ("sig_cnt", "<u2"),
                                  ("ed_code", "i1"), ("_pad", "u1", (7,))])          # fdgpu_precompile_info_t
PRECOMPILE_WALK_DTYPE = np.dtype([("sig0", "<u4"), ("sig_cnt", "<u2"), ("instr_idx", "<u2"), ("rec_idx", "<u2"),
                                  ("ed_instr_cnt", "<u2"), ("code", "i1"), ("_pad", "u1", (3,))])   # fdgpu_precompile_walk_t
CODE_PRECOMPILE_DATA_SIZE = -70     # FDGPU_CODE_PRECOMPILE_DATA_SIZE
CODE_PRECOMPILE_DATA_OFFSET = -71   # FDGPU_CODE_PRECOMPILE_DATA_OFFSET
CODE_PRECOMPILE_SIGNATURE = -72     # FDGPU_CODE_PRECOMPILE_SIGNATURE
CODE_PRECOMPILE_CAP = -73           # FDGPU_CODE_PRECOMPILE_CAP


# include/fd_secp256k1_gpu.h
SECP256K1_FAIL_ON_BAD_COUNT = 1     # FDGPU_SECP256K1_FAIL_ON_BAD_COUNT
SECP256K1_ERR_RECID = -1            # FDGPU_SECP256K1_ERR_RECID
SECP256K1_ERR_RANGE = -2            # FDGPU_SECP256K1_ERR_RANGE
SECP256K1_ERR_POINT = -3            # FDGPU_SECP256K1_ERR_POINT
SECP256K1_ERR_INFINITY = -4         # FDGPU_SECP256K1_ERR_INFINITY
SECP256K1_ERR_ADDRESS = -5          # FDGPU_SECP256K1_ERR_ADDRESS
SECP256K1_OPS_IN, SECP256K1_OPS_OUT = 49, 17    # csrc/fdgpu_secp256k1.h: words per item of debug_secp256k1_ops


def secp256k1_sig_bound(sz):
    """fdgpu_secp256k1_sig_bound: the most records a transaction of sz bytes can emit."""
    return int(_lib.lib().fdgpu_secp256k1_sig_bound(int(sz)))


def precompile_sig_bound(sz):
    """fdgpu_precompile_sig_bound: the most records a transaction of sz bytes can emit."""
    return int(_lib.lib().fdgpu_precompile_sig_bound(int(sz)))


def poh_chunk():
    """fdgpu_poh_chunk: hashes a lane of the chain kernel runs between two
    looks at the entry queue."""
    return int(_lib.lib().fdgpu_poh_chunk())


def bcomb_dims():
    """fdgpu_bcomb_dim: the fixed-base comb's shape: radix bits, tables,
    entries per table, u32 per entry, entries per chunk of the table build."""
    L = _lib.lib()
    return {k: int(L.fdgpu_bcomb_dim(i)) for i, k in enumerate(("w", "ndig", "entries", "stride", "chunk"))}


def ge_ops_shape():
    """(u32 per input record, results per record) of debug_ge_ops."""
    L = _lib.lib()
    return int(L.fdgpu_test_ge_in_words()), int(L.fdgpu_test_ge_results())


def _poh_arrays(arena, entries, sig_offs):
    return (np.ascontiguousarray(arena, dtype=np.uint8), np.ascontiguousarray(entries, dtype=POH_DTYPE),
            np.ascontiguousarray(sig_offs, dtype=np.uint32))


def verify(msg, sig, public_key, sha=None):
    """fd_ed25519_verify: returns SUCCESS or an ERR_* code."""
    msg = bytes(msg)
    sig, public_key = bytes(sig), bytes(public_key)
    if len(sig) != 64 or len(public_key) != 32:
        raise ValueError("sig must be 64 bytes and public_key 32 bytes")
    return _lib.lib().fd_ed25519_verify(msg, len(msg), sig, public_key, None)


def verify_batch_single_msg(msg, signatures, pubkeys, shas, batch_sz):
    """fd_ed25519_verify_batch_single_msg: batch_sz in [1,16] else ERR_SIG."""
    msg = bytes(msg)
    signatures, pubkeys = bytes(signatures), bytes(pubkeys)
    n = int(batch_sz)
    if n < 0 or n > 255:
        raise ValueError("batch_sz is a uchar")
    if 1 <= n <= 16 and (len(signatures) < 64 * n or len(pubkeys) < 32 * n):
        raise ValueError("signatures/pubkeys shorter than batch_sz records")
    return _lib.lib().fd_ed25519_verify_batch_single_msg(msg, len(msg), signatures, pubkeys, None, n)


def sync_stats():
    """Counters of the synchronous API (fdgpu_sync_stats): calls, the GPU
    batches concurrent calls were coalesced into, engine failures answered
    with ERR_SIG."""
    import ctypes as c
    v = [c.c_uint64() for _ in range(3)]
    _lib.lib().fdgpu_sync_stats(*[c.byref(x) for x in v])
    return {"calls": v[0].value, "batches": v[1].value, "errors": v[2].value}


def strerror(err):
    """fd_ed25519_strerror."""
    return _lib.lib().fd_ed25519_strerror(int(err)).decode()


def expand_txns(txns):
    """Per-signature and per-transaction descriptors for the device path
    (the same expansion the engine's submit performs on the host)."""
    txns = np.asarray(txns, dtype=TXN_DTYPE)
    cnt = txns["sig_cnt"].astype(np.int64)
    valid = (cnt >= 1) & (cnt <= 16)
    used = np.where(valid, cnt, 0)
    sig0 = np.zeros(len(txns), dtype=np.int64)
    if len(txns):
        sig0[1:] = np.cumsum(used)[:-1]
    n_sig = int(used.sum())
    tdesc = np.zeros(len(txns), dtype=TXN_DESC_DTYPE)
    tdesc["sig0"] = sig0
    tdesc["sig_cnt"] = used
    sdesc = np.zeros(n_sig, dtype=SIG_DESC_DTYPE)
    t_of_sig = np.repeat(np.arange(len(txns)), used)
    j = np.arange(n_sig) - sig0[t_of_sig]
    sdesc["msg_off"] = txns["msg_off"][t_of_sig]
    sdesc["msg_sz"] = txns["msg_sz"][t_of_sig]
    sdesc["sig_off"] = txns["sig_off"][t_of_sig] + 64 * j
    sdesc["pub_off"] = txns["pub_off"][t_of_sig] + 32 * j
    return sdesc, tdesc


class VerifyEngine:
    """One engine per GPU: pinned double-buffered rings, HIP streams, and the
    verify kernels.  submit()/poll() is the asynchronous batch API;
    verify_txns() is submit + blocking poll."""

    def __init__(self, device=0, max_txn=1 << 16, max_sig=None, max_arena=None, ring_depth=2, ref_mapping=False,
                 bucket=True, full_path=False, key_cache=False, pair=False, pair_auto=False, merge=False,
                 spread=False, spread_auto=False):
        L = _lib.lib()
        # max_sig default: 12 signatures per txn (FD_TXN_ACTUAL_SIG_MAX), as the engine's own default
        self.max_sig = max_sig or 12 * max_txn
        flags = ((FLAG_REF_MAPPING if ref_mapping else 0) | (0 if bucket else FLAG_NO_BUCKET) |
                 (FLAG_FULL_PATH if full_path else 0) | (FLAG_KEY_CACHE if key_cache else 0) |
                 (FLAG_PAIR if pair else 0) | (FLAG_PAIR_AUTO if pair_auto else 0) | (FLAG_MERGE if merge else 0) |
                 (FLAG_SPREAD if spread else 0) | (FLAG_SPREAD_AUTO if spread_auto else 0))
        cfg = _lib.FdgpuCfg(max_txn, self.max_sig, max_arena or 1232 * max_txn, ring_depth, flags)
        self._cfg = cfg
        self.max_arena = cfg.max_arena
        self._h = L.fdgpu_engine_open(int(device), ctypes.byref(cfg))
        if not self._h:
            raise RuntimeError(f"fdgpu_engine_open({device}) failed: {_lib.last_error()}")
        self.device = device
        self._pending = {}

    def reserve(self, n_sig=0):
        """fdgpu_engine_reserve: size every ring slot for batches of up to
        n_sig signatures (0: max_sig) now, so no batch allocates inside the
        pipeline (call with nothing in flight)."""
        r = _lib.lib().fdgpu_engine_reserve(self._h, int(n_sig))
        if r:
            raise RuntimeError(f"fdgpu_engine_reserve failed: {r} ({_lib.last_error()})")

    def host_register(self, buf):
        """Registers a long-lived host buffer (numpy array) for direct DMA:
        batches whose arena lies inside it upload with no staging copy
        (fdgpu_host_register)."""
        arr = np.asarray(buf)
        r = _lib.lib().fdgpu_host_register(self._h, arr.ctypes.data, arr.nbytes)
        if r:
            raise RuntimeError(f"fdgpu_host_register failed: {r} ({_lib.last_error()})")

    def host_unregister(self, buf):
        r = _lib.lib().fdgpu_host_unregister(self._h, np.asarray(buf).ctypes.data)
        if r:
            raise RuntimeError(f"fdgpu_host_unregister failed: {r} ({_lib.last_error()})")

    def close(self):
        if self._h:
            _lib.lib().fdgpu_engine_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        g, b, w = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64()
        _lib.lib().fdgpu_engine_info(self._h, ctypes.byref(g), ctypes.byref(b), ctypes.byref(w))
        return {"resident_blocks": g.value, "block_threads": b.value, "ws_bytes": w.value}

    def submit(self, arena, txns):
        arena = np.ascontiguousarray(arena, dtype=np.uint8)
        txns = np.ascontiguousarray(txns, dtype=TXN_DTYPE)
        tk = _lib.lib().fdgpu_submit(self._h, arena.ctypes.data, arena.size, txns.ctypes.data, len(txns))
        if tk < 0:
            raise RuntimeError(f"fdgpu_submit failed ({tk}): {_lib.last_error()}")
        self._pending[tk] = len(txns)
        return tk

    def poll(self, ticket, blocking=True):
        n = self._pending.get(ticket)
        if n is None:
            raise KeyError(ticket)
        out = np.zeros(max(n, 1), dtype=np.int8)
        rc = _lib.lib().fdgpu_poll(self._h, ticket, out.ctypes.data, 1 if blocking else 0)
        if rc == 1:
            return None
        if rc != 0:
            raise RuntimeError(f"fdgpu_poll failed ({rc}): {_lib.last_error()}")
        del self._pending[ticket]
        return out[:n]

    def verify_txns(self, arena, txns):
        return self.poll(self.submit(arena, txns), blocking=True)

    def submit_frags(self, arena, frags, trailer_sz):
        """fdgpu_submit_frags: raw payloads parsed on the GPU; frags is a
        FRAG_EX_DTYPE array ({off, sz, tr_off, tr_cap})."""
        arena = np.ascontiguousarray(arena, dtype=np.uint8)
        frags = np.ascontiguousarray(frags, dtype=FRAG_EX_DTYPE)
        tk = _lib.lib().fdgpu_submit_frags(self._h, arena.ctypes.data, arena.size, frags.ctypes.data, len(frags),
                                           int(trailer_sz))
        if tk < 0:
            raise RuntimeError(f"fdgpu_submit_frags failed ({tk}): {_lib.last_error()}")
        self._pending[tk] = (len(frags), int(trailer_sz))
        return tk

    def poll_frags(self, ticket, blocking=True):
        """-> (codes int8[n], trailers uint8[trailer_sz]) or None while pending."""
        n, tsz = self._pending[ticket]
        codes = np.zeros(max(n, 1), dtype=np.int8)
        tr = np.zeros(max(tsz, 1), dtype=np.uint8)
        rc = _lib.lib().fdgpu_poll_frags(self._h, ticket, codes.ctypes.data, tr.ctypes.data, 1 if blocking else 0)
        if rc == 1:
            return None
        if rc != 0:
            raise RuntimeError(f"fdgpu_poll_frags failed ({rc}): {_lib.last_error()}")
        del self._pending[ticket]
        return codes[:n], tr[:tsz]

    def submit_frags_io(self, frags, out, out_sz, hash_seed, links=None):
        """fdgpu_submit_frags_io: payloads read by the device where they lie
        (frags: FRAG_IO_DTYPE {src host address, sz, out_off, out_cap, link,
        seq}, every src inside a registered buffer), out frags written to
        `out` (a registered numpy buffer) [0, out_sz).  links: (mcache
        address, depth) per in link; a frag with link = i + 1 has links[i]'s
        line of its seq re-read by the device after its payload
        (FDGPU_CODE_LAPPED when republished)."""
        frags = np.ascontiguousarray(frags, dtype=FRAG_IO_DTYPE)
        out = np.asarray(out)
        if out_sz > out.nbytes:
            raise ValueError("out_sz exceeds the out buffer")
        lk = np.array(list(links or []), dtype=LINK_DTYPE)
        tk = _lib.lib().fdgpu_submit_frags_io(self._h, frags.ctypes.data, len(frags), out.ctypes.data, int(out_sz),
                                              int(hash_seed), lk.ctypes.data if len(lk) else None, len(lk))
        if tk < 0:
            raise RuntimeError(f"fdgpu_submit_frags_io failed ({tk}): {_lib.last_error()}")
        self._pending[tk] = (len(frags), frags)
        return tk

    def poll_frags_io(self, ticket, blocking=True):
        """-> (codes int8[n], tags uint64[n], out_szs uint16[n]) or None while pending."""
        n, _ = self._pending[ticket]
        codes = np.zeros(max(n, 1), dtype=np.int8)
        tags = np.zeros(max(n, 1), dtype=np.uint64)
        osz = np.zeros(max(n, 1), dtype=np.uint16)
        rc = _lib.lib().fdgpu_poll_frags_io(self._h, ticket, codes.ctypes.data, tags.ctypes.data, osz.ctypes.data,
                                            1 if blocking else 0)
        if rc == 1:
            return None
        if rc != 0:
            raise RuntimeError(f"fdgpu_poll_frags_io failed ({rc}): {_lib.last_error()}")
        del self._pending[ticket]
        return codes[:n], tags[:n], osz[:n]

    def submit_shreds(self, arena, shreds, expected_version):
        """fdgpu_submit_shreds: raw Merkle shreds (SHRED_DTYPE {off, sz,
        pub_off}) checked, hashed to their roots and verified on the GPU."""
        arena = np.ascontiguousarray(arena, dtype=np.uint8)
        shreds = np.ascontiguousarray(shreds, dtype=SHRED_DTYPE)
        tk = _lib.lib().fdgpu_submit_shreds(self._h, arena.ctypes.data, arena.size, shreds.ctypes.data, len(shreds),
                                            int(expected_version))
        if tk < 0:
            raise RuntimeError(f"fdgpu_submit_shreds failed ({tk}): {_lib.last_error()}")
        self._pending[tk] = len(shreds)
        return tk

    def poll_shreds(self, ticket, blocking=True):
        """-> (codes int8[n], roots uint8[n, 32]) or None while pending."""
        n = self._pending[ticket]
        codes = np.zeros(max(n, 1), dtype=np.int8)
        roots = np.zeros((max(n, 1), 32), dtype=np.uint8)
        rc = _lib.lib().fdgpu_poll_shreds(self._h, ticket, codes.ctypes.data, roots.ctypes.data, 1 if blocking else 0)
        if rc == 1:
            return None
        if rc != 0:
            raise RuntimeError(f"fdgpu_poll_shreds failed ({rc}): {_lib.last_error()}")
        del self._pending[ticket]
        return codes[:n], roots[:n]

    def verify_shreds(self, arena, shreds, expected_version):
        return self.poll_shreds(self.submit_shreds(arena, shreds, expected_version), blocking=True)

    def submit_shred_sets(self, arena, shreds, expected_version):
        """fdgpu_submit_shred_sets: every shred of a batch (SET_SHRED_DTYPE
        {off, sz, pub_off, known_off}), one signature verified per distinct
        (signature, root, leader key), shreds with a known root held against
        it."""
        arena = np.ascontiguousarray(arena, dtype=np.uint8)
        shreds = np.ascontiguousarray(shreds, dtype=SET_SHRED_DTYPE)
        tk = _lib.lib().fdgpu_submit_shred_sets(self._h, arena.ctypes.data, arena.size, shreds.ctypes.data, len(shreds),
                                                int(expected_version))
        if tk < 0:
            raise RuntimeError(f"fdgpu_submit_shred_sets failed ({tk}): {_lib.last_error()}")
        self._pending[tk] = len(shreds)
        return tk

    def poll_shred_sets(self, ticket, blocking=True, want_rep=True):
        """-> (codes int8[n], roots uint8[n, 32], rep uint32[n], lanes) or None
        while pending; want_rep False: rep and lanes are not asked for (None)."""
        n = self._pending[ticket]
        codes = np.zeros(max(n, 1), dtype=np.int8)
        roots = np.zeros((max(n, 1), 32), dtype=np.uint8)
        rep = np.zeros(max(n, 1), dtype=np.uint32) if want_rep else None
        lanes = ctypes.c_uint64(0)
        rc = _lib.lib().fdgpu_poll_shred_sets(self._h, ticket, codes.ctypes.data, roots.ctypes.data,
                                              rep.ctypes.data if want_rep else None,
                                              ctypes.byref(lanes) if want_rep else None, 1 if blocking else 0)
        if rc == 1:
            return None
        if rc != 0:
            raise RuntimeError(f"fdgpu_poll_shred_sets failed ({rc}): {_lib.last_error()}")
        del self._pending[ticket]
        return codes[:n], roots[:n], (rep[:n] if want_rep else None), (int(lanes.value) if want_rep else None)

    def verify_shred_sets(self, arena, shreds, expected_version):
        return self.poll_shred_sets(self.submit_shred_sets(arena, shreds, expected_version), blocking=True)

    def submit_precompiles(self, arena, txns):
        """fdgpu_submit_precompiles: raw transactions (PRECOMPILE_DTYPE {off,
        sz, sig_cap}) parsed, their Ed25519 precompile instructions walked
        and every record verified on the GPU."""
        arena = np.ascontiguousarray(arena, dtype=np.uint8)
        txns = np.ascontiguousarray(txns, dtype=PRECOMPILE_DTYPE)
        tk = _lib.lib().fdgpu_submit_precompiles(self._h, arena.ctypes.data, arena.size, txns.ctypes.data, len(txns))
        if tk < 0:
            raise RuntimeError(f"fdgpu_submit_precompiles failed ({tk}): {_lib.last_error()}")
        self._pending[tk] = len(txns)
        return tk

    def poll_precompiles(self, ticket, blocking=True):
        """-> (codes int8[n], info PRECOMPILE_INFO_DTYPE[n]) or None while pending."""
        n = self._pending[ticket]
        codes = np.zeros(max(n, 1), dtype=np.int8)
        info = np.zeros(max(n, 1), dtype=PRECOMPILE_INFO_DTYPE)
        rc = _lib.lib().fdgpu_poll_precompiles(self._h, ticket, codes.ctypes.data, info.ctypes.data,
                                               1 if blocking else 0)
        if rc == 1:
            return None
        if rc != 0:
            raise RuntimeError(f"fdgpu_poll_precompiles failed ({rc}): {_lib.last_error()}")
        del self._pending[ticket]
        return codes[:n], info[:n]

    def verify_precompiles(self, arena, txns):
        return self.poll_precompiles(self.submit_precompiles(arena, txns), blocking=True)

    def submit_secp256k1(self, arena, txns, flags=0):
        """fdgpu_submit_secp256k1: raw transactions (PRECOMPILE_DTYPE {off,
        sz, sig_cap}) parsed, their secp256k1 precompile instructions walked
        and every record checked on the GPU."""
        arena = np.ascontiguousarray(arena, dtype=np.uint8)
        txns = np.ascontiguousarray(txns, dtype=PRECOMPILE_DTYPE)
        tk = _lib.lib().fdgpu_submit_secp256k1(self._h, arena.ctypes.data, arena.size, txns.ctypes.data, len(txns),
                                               int(flags))
        if tk < 0:
            raise RuntimeError(f"fdgpu_submit_secp256k1 failed ({tk}): {_lib.last_error()}")
        self._pending[tk] = len(txns)
        return tk

    def poll_secp256k1(self, ticket, blocking=True):
        """-> (codes int8[n], info PRECOMPILE_INFO_DTYPE[n]) or None while pending."""
        n = self._pending[ticket]
        codes = np.zeros(max(n, 1), dtype=np.int8)
        info = np.zeros(max(n, 1), dtype=PRECOMPILE_INFO_DTYPE)
        rc = _lib.lib().fdgpu_poll_secp256k1(self._h, ticket, codes.ctypes.data, info.ctypes.data, 1 if blocking else 0)
        if rc == 1:
            return None
        if rc != 0:
            raise RuntimeError(f"fdgpu_poll_secp256k1 failed ({rc}): {_lib.last_error()}")
        del self._pending[ticket]
        return codes[:n], info[:n]

    def verify_secp256k1(self, arena, txns, flags=0):
        return self.poll_secp256k1(self.submit_secp256k1(arena, txns, flags), blocking=True)

    def submit_poh(self, arena, entries, sig_offs, hash_cnt_cap):
        """fdgpu_submit_poh: a block's PoH entries (POH_DTYPE; sig_offs: the
        arena offsets of their signatures) hashed, rooted, mixed and compared
        on the GPU."""
        arena, entries, sig_offs = _poh_arrays(arena, entries, sig_offs)
        tk = _lib.lib().fdgpu_submit_poh(self._h, arena.ctypes.data, arena.size, entries.ctypes.data, len(entries),
                                         sig_offs.ctypes.data, len(sig_offs), int(hash_cnt_cap))
        if tk < 0:
            raise RuntimeError(f"fdgpu_submit_poh failed ({tk}): {_lib.last_error()}")
        self._pending[tk] = len(entries)
        return tk

    def poll_poh(self, ticket, blocking=True):
        """-> (codes int8[n], hashes uint8[n, 32]) or None while pending."""
        n = self._pending[ticket]
        codes = np.zeros(max(n, 1), dtype=np.int8)
        hashes = np.zeros((max(n, 1), 32), dtype=np.uint8)
        rc = _lib.lib().fdgpu_poll_poh(self._h, ticket, codes.ctypes.data, hashes.ctypes.data, 1 if blocking else 0)
        if rc == 1:
            return None
        if rc != 0:
            raise RuntimeError(f"fdgpu_poll_poh failed ({rc}): {_lib.last_error()}")
        del self._pending[ticket]
        return codes[:n], hashes[:n]

    def verify_poh(self, arena, entries, sig_offs, hash_cnt_cap):
        return self.poll_poh(self.submit_poh(arena, entries, sig_offs, hash_cnt_cap), blocking=True)

    def verify_device(self, d_arena, d_sig_desc, n_sig, d_txn_desc, n_txn, d_sig_codes, d_txn_codes, stream=0):
        """Device-resident path; all pointers are device addresses (ints)."""
        rc = _lib.lib().fdgpu_verify_device(self._h, d_arena, d_sig_desc, n_sig, d_txn_desc, n_txn,
                                            d_sig_codes, d_txn_codes, stream or None)
        if rc != 0:
            raise RuntimeError(f"fdgpu_verify_device failed ({rc}): {_lib.last_error()}")

    def upload(self, arena, txns):
        """Stage a batch in HBM once (DeviceBatch); verify it any number of times."""
        return DeviceBatch(self, arena, txns)

    def upload_frags(self, arena, frags):
        """Raw transaction payloads in HBM (FragBatch): each verify parses
        them on the GPU (fdgpu_dev_batch_upload_frags)."""
        return FragBatch(self, arena, frags)

    def sync(self):
        self._chk(_lib.lib().fdgpu_sync(self._h), "fdgpu_sync")

    # ---- per-stage diagnostics (parity tests) ----
    def _chk(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): {_lib.last_error()}")

    def debug_fe_ops(self, ab):
        ab = np.ascontiguousarray(ab, dtype=np.uint8).reshape(-1, 64)
        out = np.zeros((len(ab), 8, 32), dtype=np.uint8)
        self._chk(_lib.lib().fdgpu_debug_fe_ops(self._h, ab.ctypes.data, len(ab), out.ctypes.data), "debug_fe_ops")
        return out

    def debug_decode(self, enc, ref_mapping=False):
        enc = np.ascontiguousarray(enc, dtype=np.uint8).reshape(-1, 32)
        out = np.zeros((len(enc), 72), dtype=np.uint8)
        self._chk(_lib.lib().fdgpu_debug_decode(self._h, enc.ctypes.data, len(enc), 1 if ref_mapping else 0,
                                                out.ctypes.data), "debug_decode")
        rc = out[:, 0:4].copy().view(np.int32)[:, 0]
        so = out[:, 4:8].copy().view(np.int32)[:, 0]
        return rc, so, out[:, 8:40], out[:, 40:72]

    def debug_sha512(self, arena, txns):
        arena = np.ascontiguousarray(arena, dtype=np.uint8)
        txns = np.ascontiguousarray(txns, dtype=TXN_DTYPE)
        out = np.zeros((len(txns), 64), dtype=np.uint8)
        self._chk(_lib.lib().fdgpu_debug_sha512(self._h, arena.ctypes.data, arena.size, txns.ctypes.data, len(txns),
                                                out.ctypes.data), "debug_sha512")
        return out

    def debug_sha256(self, arena, txns):
        """SHA-256 of arena[msg_off, +msg_sz) per record -> uint8[n, 32] (the shred path's hash)"""
        arena = np.ascontiguousarray(arena, dtype=np.uint8)
        txns = np.ascontiguousarray(txns, dtype=TXN_DTYPE)
        out = np.zeros((len(txns), 32), dtype=np.uint8)
        self._chk(_lib.lib().fdgpu_debug_sha256(self._h, arena.ctypes.data, arena.size, txns.ctypes.data, len(txns),
                                                out.ctypes.data), "debug_sha256")
        return out

    def debug_shred_roots(self, arena, shreds, expected_version):
        """The shred checks and Merkle roots alone -> (ok int8[n]: 0 or
        CODE_SHRED_REJECT, roots uint8[n, 32])"""
        arena = np.ascontiguousarray(arena, dtype=np.uint8)
        shreds = np.ascontiguousarray(shreds, dtype=SHRED_DTYPE)
        ok = np.zeros(len(shreds), dtype=np.int8)
        roots = np.zeros((len(shreds), 32), dtype=np.uint8)
        self._chk(_lib.lib().fdgpu_debug_shred_roots(self._h, arena.ctypes.data, arena.size, shreds.ctypes.data,
                                                     len(shreds), int(expected_version), ok.ctypes.data,
                                                     roots.ctypes.data), "debug_shred_roots")
        return ok, roots

    def debug_shred_time(self, arena, shreds, expected_version, iters=5):
        """-> (ingest_ms, verify_ms): mean device time of the batch's ingest
        and of its verify, the batch resident in HBM"""
        arena = np.ascontiguousarray(arena, dtype=np.uint8)
        shreds = np.ascontiguousarray(shreds, dtype=SHRED_DTYPE)
        a, v = ctypes.c_double(), ctypes.c_double()
        self._chk(_lib.lib().fdgpu_debug_shred_time(self._h, arena.ctypes.data, arena.size, shreds.ctypes.data,
                                                    len(shreds), int(expected_version), int(iters), ctypes.byref(a),
                                                    ctypes.byref(v)), "debug_shred_time")
        return a.value, v.value

    def debug_shred_sets_time(self, arena, shreds, expected_version, iters=5):
        """-> (ingest_ms, verify_ms): mean device time of a set batch's ingest
        and dedup and of its verify, the batch resident in HBM"""
        arena = np.ascontiguousarray(arena, dtype=np.uint8)
        shreds = np.ascontiguousarray(shreds, dtype=SET_SHRED_DTYPE)
        a, v = ctypes.c_double(), ctypes.c_double()
        self._chk(_lib.lib().fdgpu_debug_shred_sets_time(self._h, arena.ctypes.data, arena.size, shreds.ctypes.data,
                                                         len(shreds), int(expected_version), int(iters), ctypes.byref(a),
                                                         ctypes.byref(v)), "debug_shred_sets_time")
        return a.value, v.value

    def debug_precompile_walk(self, arena, txns):
        """The precompile ingest alone -> (walk PRECOMPILE_WALK_DTYPE[n],
        descs SIG_DESC_DTYPE[k], pos uint32[k]: instr_idx << 16 | rec_idx),
        k the signature slots taken"""
        arena = np.ascontiguousarray(arena, dtype=np.uint8)
        txns = np.ascontiguousarray(txns, dtype=PRECOMPILE_DTYPE)
        cap = int(txns["sig_cap"].astype(np.uint64).sum())
        walk = np.zeros(len(txns), dtype=PRECOMPILE_WALK_DTYPE)
        descs = np.zeros(max(cap, 1), dtype=SIG_DESC_DTYPE)
        pos = np.zeros(max(cap, 1), dtype=np.uint32)
        k = ctypes.c_uint64()
        self._chk(_lib.lib().fdgpu_debug_precompile_walk(self._h, arena.ctypes.data, arena.size, txns.ctypes.data,
                                                         len(txns), walk.ctypes.data, descs.ctypes.data,
                                                         pos.ctypes.data, max(cap, 1), ctypes.byref(k)),
                  "debug_precompile_walk")
        return walk, descs[:k.value], pos[:k.value]

    def debug_precompile_time(self, arena, txns, iters=5):
        """-> (ingest_ms, verify_ms): mean device time of the batch's ingest
        and of its verify, the batch resident in HBM"""
        arena = np.ascontiguousarray(arena, dtype=np.uint8)
        txns = np.ascontiguousarray(txns, dtype=PRECOMPILE_DTYPE)
        a, v = ctypes.c_double(), ctypes.c_double()
        self._chk(_lib.lib().fdgpu_debug_precompile_time(self._h, arena.ctypes.data, arena.size, txns.ctypes.data,
                                                         len(txns), int(iters), ctypes.byref(a), ctypes.byref(v)),
                  "debug_precompile_time")
        return a.value, v.value

    def debug_secp256k1_walk(self, arena, txns, flags=0):
        """The secp256k1 ingest alone -> (walk PRECOMPILE_WALK_DTYPE[n],
        descs SIG_DESC_DTYPE[k] (pub_off: the address), pos uint32[k]:
        instr_idx << 16 | rec_idx), k the record slots taken"""
        arena = np.ascontiguousarray(arena, dtype=np.uint8)
        txns = np.ascontiguousarray(txns, dtype=PRECOMPILE_DTYPE)
        cap = int(txns["sig_cap"].astype(np.uint64).sum())
        walk = np.zeros(len(txns), dtype=PRECOMPILE_WALK_DTYPE)
        descs = np.zeros(max(cap, 1), dtype=SIG_DESC_DTYPE)
        pos = np.zeros(max(cap, 1), dtype=np.uint32)
        k = ctypes.c_uint64()
        self._chk(_lib.lib().fdgpu_debug_secp256k1_walk(self._h, arena.ctypes.data, arena.size, txns.ctypes.data,
                                                        len(txns), int(flags), walk.ctypes.data, descs.ctypes.data,
                                                        pos.ctypes.data, max(cap, 1), ctypes.byref(k)),
                  "debug_secp256k1_walk")
        return walk, descs[:k.value], pos[:k.value]

    def debug_keccak256(self, msgs):
        """Keccak-256 of each of msgs (bytes, at most 1232 each), one per lane -> uint8[n, 32]"""
        arena = np.frombuffer(b"".join(msgs) + b"\0", dtype=np.uint8)
        os_ = np.zeros((len(msgs), 2), dtype=np.uint32)
        at = 0
        for i, m in enumerate(msgs):
            os_[i] = (at, len(m))
            at += len(m)
        out = np.zeros((len(msgs), 32), dtype=np.uint8)
        self._chk(_lib.lib().fdgpu_debug_keccak256(self._h, arena.ctypes.data, arena.size - 1, os_.ctypes.data, len(msgs),
                                                   out.ctypes.data), "debug_keccak256")
        return out

    def debug_secp256k1_recover(self, items):
        """items: (hash32, sig64, recid) -> (codes int8[n], keys uint8[n, 64])"""
        buf = np.frombuffer(b"".join(bytes(h) + bytes(s) + bytes([r & 0xFF]) for h, s, r in items), dtype=np.uint8)
        if buf.size != 97 * len(items):
            raise ValueError("each item is 32 + 64 bytes and a recovery id")
        codes = np.zeros(len(items), dtype=np.int8)
        keys = np.zeros((len(items), 64), dtype=np.uint8)
        self._chk(_lib.lib().fdgpu_debug_secp256k1_recover(self._h, buf.ctypes.data, len(items), codes.ctypes.data,
                                                           keys.ctypes.data), "debug_secp256k1_recover")
        return codes, keys

    def debug_secp256k1_ops(self, items):
        """items: (op, a, b, c, d, e, f) of integers below 2^256 (missing
        ones 0); the operations are listed at fdgpu_debug_secp256k1_ops
        (csrc/fdgpu_secp256k1.h) -> [(flag, x, y)] as integers"""
        buf = np.zeros((len(items), SECP256K1_OPS_IN), dtype=np.uint32)
        for i, it in enumerate(items):
            buf[i, 0] = it[0]
            for k, v in enumerate(it[1:]):
                buf[i, 1 + 8 * k:9 + 8 * k] = [(v >> (32 * j)) & 0xFFFFFFFF for j in range(8)]
        out = np.zeros((len(items), SECP256K1_OPS_OUT), dtype=np.uint32)
        self._chk(_lib.lib().fdgpu_debug_secp256k1_ops(self._h, buf.ctypes.data, len(items), out.ctypes.data),
                  "debug_secp256k1_ops")
        val = lambda w: sum(int(x) << (32 * j) for j, x in enumerate(w))
        return [(int(o[0]), val(o[1:9]), val(o[9:17])) for o in out]

    def debug_secp256k1_time(self, arena, txns, flags=0, iters=5):
        """-> (ingest_ms, recover_ms): mean device time of the batch's ingest
        and of its recover kernel, the batch resident in HBM"""
        arena = np.ascontiguousarray(arena, dtype=np.uint8)
        txns = np.ascontiguousarray(txns, dtype=PRECOMPILE_DTYPE)
        a, v = ctypes.c_double(), ctypes.c_double()
        self._chk(_lib.lib().fdgpu_debug_secp256k1_time(self._h, arena.ctypes.data, arena.size, txns.ctypes.data,
                                                        len(txns), int(flags), int(iters), ctypes.byref(a),
                                                        ctypes.byref(v)), "debug_secp256k1_time")
        return a.value, v.value

    def debug_poh(self, arena, entries, sig_offs, hash_cnt_cap, grid_waves=0):
        """The PoH pipeline outside the ring, the chain kernel's grid forced
        to grid_waves waves (0: the default) -> (codes int8[n], hashes uint8[n, 32])"""
        arena, entries, sig_offs = _poh_arrays(arena, entries, sig_offs)
        codes = np.zeros(len(entries), dtype=np.int8)
        hashes = np.zeros((len(entries), 32), dtype=np.uint8)
        self._chk(_lib.lib().fdgpu_debug_poh(self._h, arena.ctypes.data, arena.size, entries.ctypes.data, len(entries),
                                             sig_offs.ctypes.data, len(sig_offs), int(hash_cnt_cap), int(grid_waves),
                                             codes.ctypes.data, hashes.ctypes.data), "debug_poh")
        return codes, hashes

    def debug_poh_time(self, arena, entries, sig_offs, hash_cnt_cap, iters=5):
        """-> (tree_ms, chain_ms): mean device time of the batch's leaves and
        roots and of its chains, the batch resident in HBM"""
        arena, entries, sig_offs = _poh_arrays(arena, entries, sig_offs)
        t, ch = ctypes.c_double(), ctypes.c_double()
        self._chk(_lib.lib().fdgpu_debug_poh_time(self._h, arena.ctypes.data, arena.size, entries.ctypes.data,
                                                  len(entries), sig_offs.ctypes.data, len(sig_offs), int(hash_cnt_cap),
                                                  int(iters), ctypes.byref(t), ctypes.byref(ch)), "debug_poh_time")
        return t.value, ch.value

    def debug_hram(self, arena, txns):
        arena = np.ascontiguousarray(arena, dtype=np.uint8)
        txns = np.ascontiguousarray(txns, dtype=TXN_DTYPE)
        out = np.zeros((len(txns), 32), dtype=np.uint8)
        self._chk(_lib.lib().fdgpu_debug_hram(self._h, arena.ctypes.data, arena.size, txns.ctypes.data, len(txns),
                                              out.ctypes.data), "debug_hram")
        return out

    def debug_sc_reduce(self, x):
        x = np.ascontiguousarray(x, dtype=np.uint8).reshape(-1, 64)
        out = np.zeros((len(x), 32), dtype=np.uint8)
        self._chk(_lib.lib().fdgpu_debug_sc_reduce(self._h, x.ctypes.data, len(x), out.ctypes.data), "debug_sc_reduce")
        return out

    def debug_hs_split(self, k):
        """k: uint8[n, 32] scalars < L -> uint32[n, 16] (|u|, |v|, ok, u_neg, v_neg, bits)"""
        k = np.ascontiguousarray(k, dtype=np.uint8).reshape(-1, 32)
        out = np.zeros((len(k), 16), dtype=np.uint32)
        self._chk(_lib.lib().fdgpu_debug_hs_split(self._h, k.ctypes.data, len(k), out.ctypes.data), "debug_hs_split")
        return out

    def debug_fe_raw(self, fg):
        """fg: uint32[n, 20] raw limb vectors (f, g), taken as they are ->
        uint32[n, 10, 8] canonical LE words of f*g, f^2, f+g, f-g, (f-g)*g,
        -f, (-f)*g, f, f-g by 4p, (f-g by 4p)*g"""
        fg = np.ascontiguousarray(fg, dtype=np.uint32).reshape(-1, 20)
        out = np.zeros((len(fg), 10, 8), dtype=np.uint32)
        self._chk(_lib.lib().fdgpu_debug_fe_raw(self._h, fg.ctypes.data, len(fg), out.ctypes.data), "debug_fe_raw")
        return out

    def debug_ge_ops(self, rec):
        """rec: uint32[n, ge_ops_shape()[0]]: P and Q (X, Y, Z, T as 8 LE
        words each) and Q's affine niels form -> uint32[n, results, 4, 8]
        (X, Y, Z, T canonical; the results' order: csrc/fdgpu_test_kernels.hip)"""
        w_in, n_res = ge_ops_shape()
        rec = np.ascontiguousarray(rec, dtype=np.uint32).reshape(-1, w_in)
        out = np.zeros((len(rec), n_res, 4, 8), dtype=np.uint32)
        self._chk(_lib.lib().fdgpu_debug_ge_ops(self._h, rec.ctypes.data, len(rec), out.ctypes.data), "debug_ge_ops")
        return out

    def debug_sc_recode(self, s):
        """s: uint8[n, 32] scalars -> uint32[n, 16]: sc_recode16's packed
        digits (8 words), then the comb recoding's"""
        s = np.ascontiguousarray(s, dtype=np.uint8).reshape(-1, 32)
        out = np.zeros((len(s), 16), dtype=np.uint32)
        self._chk(_lib.lib().fdgpu_debug_sc_recode(self._h, s.ctypes.data, len(s), out.ctypes.data), "debug_sc_recode")
        return out

    def debug_tabpack(self, ent):
        """ent: uint32[n, 40] raw limbs of cached entries (Y+X, Y-X, 2Z, 2dT)
        -> (uint32[n, 32] the stored packed words, uint32[n, 3, 40] the limbs
        read back by atab_load, by the LDS path, and by the LDS path with neg)"""
        ent = np.ascontiguousarray(ent, dtype=np.uint32).reshape(-1, 40)
        out = np.zeros((len(ent), 160), dtype=np.uint32)
        self._chk(_lib.lib().fdgpu_debug_tabpack(self._h, ent.ctypes.data, len(ent), out.ctypes.data), "debug_tabpack")
        return out[:, :32].copy(), out[:, 32:152].reshape(-1, 3, 40).copy()

    def debug_verify_prehashed(self, arena, descs, full=False, pair=False, ref_mapping=False):
        """The verify chain at chosen k: descs (SIG_DESC_DTYPE, descriptor i =
        lane i) whose msg_off is the 8-B aligned offset of 64 B of SHA-512
        state words in arena, through the prehashed verify launch.  full:
        every lane through the fallback; pair: the two-lane kernel.
        -> (int8[n] codes, the fallback queue's final count)"""
        arena = np.ascontiguousarray(arena, dtype=np.uint8)
        descs = np.ascontiguousarray(descs, dtype=SIG_DESC_DTYPE)
        codes = np.zeros(len(descs), dtype=np.int8)
        n_full = ctypes.c_uint32(0)
        flags = (KFLAG_REF_MAP if ref_mapping else 0) | (KFLAG_FULL if full else 0) | (KFLAG_PAIR if pair else 0)
        self._chk(_lib.lib().fdgpu_debug_verify_prehashed(self._h, arena.ctypes.data, arena.size, descs.ctypes.data,
                                                          len(descs), flags, codes.ctypes.data, ctypes.byref(n_full)),
                  "debug_verify_prehashed")
        return codes, int(n_full.value)

    def debug_btab(self):
        """The engine's fixed-base comb table -> uint32[NDIG, entries, stride]"""
        d = bcomb_dims()
        out = np.zeros((d["ndig"], d["entries"], d["stride"]), dtype=np.uint32)
        self._chk(_lib.lib().fdgpu_debug_btab(self._h, 0, d["ndig"] * d["entries"], out.ctypes.data), "debug_btab")
        return out

    def debug_sig_codes(self, arena, txns):
        arena = np.ascontiguousarray(arena, dtype=np.uint8)
        txns = np.ascontiguousarray(txns, dtype=TXN_DTYPE)
        cnt = txns["sig_cnt"].astype(np.int64)
        n = int(np.where((cnt >= 1) & (cnt <= 16), cnt, 0).sum())
        out = np.zeros(max(n, 1), dtype=np.int8)
        self._chk(_lib.lib().fdgpu_debug_sig_codes(self._h, arena.ctypes.data, arena.size, txns.ctypes.data,
                                                   len(txns), out.ctypes.data), "debug_sig_codes")
        return out[:n]


class DeviceBatch:
    """A batch resident in HBM (fdgpu_dev_batch_t)."""

    def __init__(self, engine, arena, txns):
        arena = np.ascontiguousarray(arena, dtype=np.uint8)
        txns = np.ascontiguousarray(txns, dtype=TXN_DTYPE)
        self._e = engine
        self.n_txn = len(txns)
        self._b = _lib.lib().fdgpu_dev_batch_upload(engine._h, arena.ctypes.data, arena.size, txns.ctypes.data,
                                                    len(txns))
        if not self._b:
            raise RuntimeError(f"fdgpu_dev_batch_upload failed: {_lib.last_error()}")
        self.n_sig = int(_lib.lib().fdgpu_dev_batch_sig_cnt(self._b))

    def own_queue(self):
        """Give this batch its own HIP stream + workspace (verifies of
        different batches then overlap on the GPU, like ring slots)."""
        rc = _lib.lib().fdgpu_dev_batch_own_queue(self._e._h, self._b)
        if rc != 0:
            raise RuntimeError(f"fdgpu_dev_batch_own_queue failed ({rc}): {_lib.last_error()}")
        return self

    def verify(self):
        """Enqueue one verify (async on the batch's queue: the engine's
        compute stream unless own_queue() was called)."""
        rc = _lib.lib().fdgpu_dev_batch_verify(self._e._h, self._b)
        if rc != 0:
            raise RuntimeError(f"fdgpu_dev_batch_verify failed ({rc}): {_lib.last_error()}")

    def codes(self, sig_codes=False):
        t = np.zeros(max(self.n_txn, 1), dtype=np.int8)
        s = np.zeros(max(self.n_sig, 1), dtype=np.int8) if sig_codes else None
        rc = _lib.lib().fdgpu_dev_batch_codes(self._e._h, self._b, t.ctypes.data,
                                              s.ctypes.data if s is not None else None)
        if rc != 0:
            raise RuntimeError(f"fdgpu_dev_batch_codes failed ({rc}): {_lib.last_error()}")
        return (t[:self.n_txn], s[:self.n_sig]) if sig_codes else t[:self.n_txn]

    def time(self, iters):
        """HIP-event timing of `iters` back-to-back verifies: (wall_ms,
        mean verify-kernel ms, mean combine-kernel ms)."""
        import ctypes as c
        w, v, k = c.c_double(), c.c_double(), c.c_double()
        rc = _lib.lib().fdgpu_dev_batch_time(self._e._h, self._b, int(iters), c.byref(w), c.byref(v), c.byref(k))
        if rc != 0:
            raise RuntimeError(f"fdgpu_dev_batch_time failed ({rc}): {_lib.last_error()}")
        return w.value, v.value, k.value

    def free(self):
        if self._b:
            _lib.lib().fdgpu_dev_batch_free(self._e._h, self._b)
            self._b = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


FRAG_DTYPE = np.dtype([("off", "<u4"), ("sz", "<u4")])
FRAG_EX_DTYPE = np.dtype([("off", "<u4"), ("sz", "<u4"), ("tr_off", "<u4"), ("tr_cap", "<u4")])
FRAG_IO_DTYPE = np.dtype([("src", "<u8"), ("sz", "<u4"), ("out_off", "<u4"), ("out_cap", "<u4"), ("link", "<u4"),
                          ("seq", "<u8")])
LINK_DTYPE = np.dtype([("mcache", "<u8"), ("depth", "<u8")])   # fdgpu_link_t
CODE_LAPPED = -66             # FDGPU_CODE_LAPPED
CODE_TRAILER_CAP = -65        # FDGPU_CODE_TRAILER_CAP
CODE_PARSE_FAIL = -64          # FDGPU_CODE_PARSE_FAIL
TXN_MAX_SZ = 852               # FD_TXN_MAX_SZ: stride of the parsed fd_txn_t records


class FragBatch(DeviceBatch):
    """Raw payloads resident in HBM (fdgpu_dev_batch_upload_frags): verify()
    runs fd_txn_parse, the signature-count scan and the descriptor expansion
    on the GPU before the verify kernels."""

    def __init__(self, engine, arena, frags):
        arena = np.ascontiguousarray(arena, dtype=np.uint8)
        frags = np.ascontiguousarray(frags, dtype=FRAG_DTYPE)
        self._e = engine
        self.n_txn = len(frags)
        self._b = _lib.lib().fdgpu_dev_batch_upload_frags(engine._h, arena.ctypes.data, arena.size,
                                                          frags.ctypes.data, len(frags))
        if not self._b:
            raise RuntimeError(f"fdgpu_dev_batch_upload_frags failed: {_lib.last_error()}")
        sz = frags["sz"].astype(np.int64)
        self.sig_bound = int(np.where(sz >= 134, np.minimum(16, (sz - 38) // 96), 0).sum())   # fdgpu_frag_sig_bound
        self.n_sig = self.sig_bound

    def codes(self, sig_codes=False):
        out = super().codes(sig_codes)
        self.n_sig = int(_lib.lib().fdgpu_dev_batch_sig_cnt(self._b))
        if sig_codes:
            return out[0], out[1][:self.n_sig]
        return out

    def txns(self, records=True):
        """(parsed fd_txn_t records uint8[n, 852] or None, footprints uint16[n]; 0 = not a txn)"""
        out = np.zeros((max(self.n_txn, 1), TXN_MAX_SZ), dtype=np.uint8) if records else None
        sz = np.zeros(max(self.n_txn, 1), dtype=np.uint16)
        rc = _lib.lib().fdgpu_dev_batch_txns(self._e._h, self._b, out.ctypes.data if records else None,
                                             sz.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"fdgpu_dev_batch_txns failed ({rc}): {_lib.last_error()}")
        return (out[:self.n_txn] if records else None), sz[:self.n_txn]

    def time2(self, iters):
        """HIP-event timing: (wall_ms, mean ingest ms (parse + scan + expand),
        mean verify-kernel ms, mean combine ms)."""
        import ctypes as c
        w, g, v, k = c.c_double(), c.c_double(), c.c_double(), c.c_double()
        rc = _lib.lib().fdgpu_dev_batch_time2(self._e._h, self._b, int(iters), c.byref(w), c.byref(g), c.byref(v),
                                              c.byref(k))
        if rc != 0:
            raise RuntimeError(f"fdgpu_dev_batch_time2 failed ({rc}): {_lib.last_error()}")
        return w.value, g.value, v.value, k.value
