"""Python reference for the Ed25519 precompile check (tests only).

Three parts:
  * a builder of legacy and v0 transactions with arbitrary instruction lists,
    which returns the bytes and each instruction's data offset and size;
  * the rules of fd_executor_verify_precompiles (reference
    src/flamenco/runtime/fd_executor.c:252-270) and fd_precompile_ed25519_verify
    (src/flamenco/runtime/program/fd_precompiles.c:73-206) restated over that
    model, independent of the C source (firedancer_amd/csrc/fdt_precompile.h);
  * a case generator with a counter-based RNG.

This is a restatement pinned by line citations, not by running the reference:
no reference binary for the precompile check exists in this repository.
Verdicts come from a per-record verify callable (the tests pass oracle.verify).
"""
import hashlib
import struct

import numpy as np

CODE_PARSE_FAIL = -64
CODE_DATA_SIZE, CODE_DATA_OFFSET, CODE_SIGNATURE, CODE_CAP = -70, -71, -72, -73
NONE = 0xFFFF
ED25519_NAME = "Ed25519SigVerify111111111111111111111111111"
SECP256K1_NAME = "KeccakSecp256k11111111111111111111111111111"
ED25519_ID_HEX = "037d46d67c93fbbe12f9428f838d40ff0570744927f48a64fcca704480000000"
MTU = 1232
_B58 = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz"


def b58decode32(s):
    """A base58 (Bitcoin alphabet) string -> 32 bytes."""
    v = 0
    for ch in s:
        v = v * 58 + _B58.index(ch)
    return v.to_bytes(32, "big")


ED25519_ID = b58decode32(ED25519_NAME)
SECP256K1_ID = b58decode32(SECP256K1_NAME)


class Rng:
    """Counter-based: draw k is SHA-256(seed || k), so a case's bytes do not
    depend on what was drawn before it under another label."""

    def __init__(self, seed):
        self.seed, self.k = str(seed).encode(), 0

    def bytes(self, n):
        out = b""
        while len(out) < n:
            out += hashlib.sha256(self.seed + struct.pack("<Q", self.k)).digest()
            self.k += 1
        return out[:n]

    def below(self, n):
        return int.from_bytes(self.bytes(8), "little") % n


# ---------------------------------------------------------------- builder

def cu16(v):
    """compact-u16 (fd_compact_u16.h), minimally encoded"""
    if v < 0x80:
        return bytes([v])
    if v < 0x4000:
        return bytes([(v & 0x7F) | 0x80, v >> 7])
    return bytes([(v & 0x7F) | 0x80, ((v >> 7) & 0x7F) | 0x80, v >> 14])


def build_txn(accts, instrs, v0=False, luts=(), sigs=None, blockhash=None):
    """accts: 32-byte static keys (accts[0] the fee payer); instrs: (program
    index, account index bytes, data); luts (v0): (32-byte key, writable index
    bytes, readonly index bytes).  One signer.  -> (bytes, [(data_off,
    data_sz)] per instruction)"""
    sigs = sigs if sigs is not None else [bytes(64)]
    out = bytearray(cu16(len(sigs)))
    for s in sigs:
        out += s
    if v0:
        out += b"\x80"
    out += bytes([len(sigs), 0, 0]) + cu16(len(accts))
    for a in accts:
        assert len(a) == 32
        out += a
    out += blockhash if blockhash is not None else bytes(range(32))
    out += cu16(len(instrs))
    offs = []
    for prog, ia, data in instrs:
        out += bytes([prog]) + cu16(len(ia)) + bytes(ia) + cu16(len(data))
        offs.append((len(out), len(data)))
        out += bytes(data)
    if v0:
        out += cu16(len(luts))
        for key, w, r in luts:
            out += key + cu16(len(w)) + bytes(w) + cu16(len(r)) + bytes(r)
    return bytes(out), offs


def record(sig_off, sig_ix, pub_off, pub_ix, msg_off, msg_sz, msg_ix):
    """fd_ed25519_signature_offsets_t: seven little-endian u16"""
    return struct.pack("<7H", sig_off, sig_ix, pub_off, pub_ix, msg_off, msg_sz, msg_ix)


def table(recs, cnt=None, pad=0):
    return bytes([len(recs) if cnt is None else cnt, pad]) + b"".join(recs)


# ------------------------------------------------------------------ rules

def walk(accts, instrs, data_offs):
    """The structural half (fd_executor.c:255-262, fd_precompiles.c:121-196).
    -> (code, instr_idx, rec_idx, ed_instr_cnt, recs) with recs the records
    that resolve before the first structural failure, in order: (instr_idx,
    rec_idx, sig_off, pub_off, msg_off, msg_sz) in payload offsets."""
    code, fi, fr, ed_cnt, recs = 0, NONE, NONE, 0, []
    n = len(instrs)

    def resolve(cur, ix, off, size):                       # fd_precompiles.c:73-111
        k = cur if ix == 0xFFFF else ix                    # :88
        if k >= n:                                         # :97
            return None
        if off + size > len(instrs[k][2]):                 # :106
            return None
        return data_offs[k][0] + off

    for j, (prog, _, data) in enumerate(instrs):
        if accts[prog] != ED25519_ID:                      # fd_executor.c:259; secp256k1 is not restated
            continue
        ed_cnt += 1
        if code:                                           # the reference returned at the first failure
            continue
        if len(data) < 16:                                 # :133
            if len(data) == 2 and data[0] == 0:            # :134
                continue
            code, fi = CODE_DATA_SIZE, j                   # :137
            continue
        cnt = data[0]                                      # :140
        if cnt == 0 or len(data) < 14 * cnt + 2:           # :141-149
            code, fi = CODE_DATA_SIZE, j
            continue
        for i in range(cnt):                               # :152
            so, si, po, pi, mo, ms, mi = struct.unpack_from("<7H", data, 2 + 14 * i)
            s = resolve(j, si, so, 64)                     # :161-167
            p = resolve(j, pi, po, 32) if s is not None else None    # :175-181
            m = resolve(j, mi, mo, ms) if p is not None else None    # :190-196
            if m is None:
                code, fi, fr = CODE_DATA_OFFSET, j, i
                break
            recs.append((j, i, s, p, m, ms))
    return code, fi, fr, ed_cnt, recs


def verdict(payload, model, verify):
    """-> (code, (instr_idx, rec_idx, ed_instr_cnt, sig_cnt, ed_code), recs).
    model None: the payload does not parse.  The first failing event in
    (instruction, record) order decides (:167-202): every emitted record lies
    before the structural failure, so the first failed verify wins."""
    if model is None:
        return CODE_PARSE_FAIL, (NONE, NONE, 0, 0, 0), []
    accts, instrs, data_offs = model
    code, fi, fr, ed_cnt, recs = walk(accts, instrs, data_offs)
    for (j, i, s, p, m, ms) in recs:
        c = verify(payload[m:m + ms], payload[s:s + 64], payload[p:p + 32])      # :201
        if c:
            return CODE_SIGNATURE, (j, i, ed_cnt, len(recs), c), recs
    return code, (fi, fr, ed_cnt, len(recs), 0), recs


def sig_bound(sz):
    """The bound of fdt_precompile_sig_bound, restated: 166 bytes of smallest
    transaction, 5 of instruction and table header, 14 a record."""
    s = min(sz, MTU)
    return (s - 171) // 14 if s >= 185 else 0


# ------------------------------------------------------------------ cases

class Case:
    def __init__(self, name, payload, model):
        self.name, self.payload, self.model = name, payload, model


class Gen:
    """Builds cases.  sign(prv, msg) -> (pub, sig)."""

    def __init__(self, sign, seed="precompile"):
        self.sign, self.rng = sign, Rng(seed)
        self.payer, self.other = self.rng.bytes(32), self.rng.bytes(32)

    def triple(self, msg_len, bad=None):
        """(sig, pub, msg), valid unless bad: 'S' (S >= L), 'key' (a
        small-order key), 'R' (another R), 'msg' (a changed message; needs
        msg_len > 0)"""
        msg = self.rng.bytes(msg_len)
        pub, sig = self.sign(self.rng.bytes(32), msg)
        if bad == "S":
            sig = sig[:32] + b"\xff" * 32
        elif bad == "key":
            pub = b"\x01" + bytes(31)
        elif bad == "R":
            sig = self.sign(self.rng.bytes(32), b"x")[1][:32] + sig[32:]
        elif bad == "msg":
            msg = bytes([msg[0] ^ 1]) + msg[1:]
        return sig, pub, msg

    def self_ix(self, lens, bads=None, idx=0xFFFF):
        """An Ed25519 instruction's data whose records point into itself
        (through index idx): table, then sig | pub | msg per record."""
        n = len(lens)
        bads = bads or [None] * n
        blobs, recs, at = b"", [], 2 + 14 * n
        for ln, bad in zip(lens, bads):
            s, p, m = self.triple(ln, bad)
            recs.append(record(at, idx, at + 64, idx, at + 96, ln, idx))
            blobs += s + p + m
            at += 96 + ln
        return table(recs) + blobs

    def case(self, name, instrs, accts=None, v0=False, luts=()):
        accts = accts if accts is not None else [self.payer, self.other, SECP256K1_ID, ED25519_ID]
        payload, offs = build_txn(accts, instrs, v0=v0, luts=luts)
        assert len(payload) <= MTU, (name, len(payload))
        return Case(name, payload, (accts, [(p, bytes(a), bytes(d)) for p, a, d in instrs], offs))


ED, SECP, OTHER = 3, 2, 1      # program indices in Gen.case's default account list


def cpu_cases(sign):
    """The CPU test's case set (the GPU parity tests run the same)."""
    g = Gen(sign)
    out = []
    add = lambda name, instrs, **kw: out.append(g.case(name, instrs, **kw))
    s, p, m = g.triple(40)
    holder = s + p + m                                         # another program's data: sig at 0, pub at 64, msg at 96
    hrec = lambda h=0, ms=40: record(0, h, 64, h, 96, ms, h)     # a record that points into holder instruction h
    # data sizes
    add("no_instr", [])
    add("no_ed_instr", [(OTHER, b"\0", holder)])
    add("sz0", [(ED, b"", b"")])
    add("sz1", [(ED, b"", b"\0")])
    add("sz2_00", [(ED, b"", b"\0\0")])
    add("sz2_0x", [(ED, b"", b"\0\x7f")])
    add("sz2_10", [(ED, b"", b"\1\0")])
    add("sz15", [(OTHER, b"", holder), (ED, b"", table([hrec()])[:15])])
    add("sz16", [(OTHER, b"", holder), (ED, b"", table([hrec()]))])
    add("sz16_pad_ignored", [(OTHER, b"", holder), (ED, b"", table([hrec()], pad=0xEE))])
    add("cnt0_sz16", [(OTHER, b"", holder), (ED, b"", table([hrec()], cnt=0))])
    add("cnt0_sz40", [(ED, b"", bytes(40))])
    add("cnt3_short", [(OTHER, b"", holder), (ED, b"", table([hrec()] * 3)[:-1])])
    add("cnt3_exact", [(OTHER, b"", holder), (ED, b"", table([hrec()] * 3))])
    add("cnt3_over", [(OTHER, b"", holder), (ED, b"", table([hrec()] * 3) + b"\x55")])
    add("cnt255", [(OTHER, b"", holder), (ED, b"", table([hrec()] * 60, cnt=255))])
    # instruction indices: each field at 0xFFFF and at the instruction's own number (0 and 1)
    add("self_ffff", [(ED, b"", g.self_ix([33]))])
    add("self_own0", [(ED, b"", g.self_ix([33], idx=0))])
    add("self_own1", [(OTHER, b"", b"zz"), (ED, b"\1\0", g.self_ix([33], idx=1))])
    d = g.self_ix([20])
    for f, name in ((1, "sig"), (3, "pub"), (6, "msg")):
        for ix, tag in ((0xFFFF, "ffff"), (0, "own"), (1, "cnt"), (2, "cnt1"), (0xFFFE, "fffe")):
            r = list(struct.unpack_from("<7H", d, 2))
            r[f] = ix
            add(f"ix_{name}_{tag}", [(ED, b"", d[:2] + struct.pack("<7H", *r) + d[16:])])
    add("ix_earlier", [(OTHER, b"", holder), (ED, b"", table([hrec(0)]))])
    add("ix_later", [(ED, b"", table([hrec(1)])), (OTHER, b"", holder)])
    add("ix_later_ed", [(ED, b"", table([hrec(1, 20)])), (ED, b"", g.self_ix([20]) + bytes(60))])
    add("ix_other_program_secp", [(ED, b"", table([hrec(1)])), (SECP, b"", holder)])
    add("ix_mixed", [(OTHER, b"", holder), (ED, b"", table([record(0, 0, 64, 2, 96, 40, 0)])), (SECP, b"", holder)])
    # offsets
    add("off_end_exact", [(OTHER, b"", holder), (ED, b"", table([record(len(holder) - 64, 0, len(holder) - 32, 0, 96, 40, 0)]))])
    for f, name, size in ((0, "sig", 64), (2, "pub", 32), (4, "msg", 40)):
        r = [0, 0, 64, 0, 96, 40, 0]
        r[f] = len(holder) - size + 1
        add(f"off_{name}_one_past", [(OTHER, b"", holder), (ED, b"", table([record(*r)]))])
        r[f] = 0xFFFF
        add(f"off_{name}_ffff", [(OTHER, b"", holder), (ED, b"", table([record(*r)]))])
    add("msg_sz_one_past", [(OTHER, b"", holder), (ED, b"", table([record(0, 0, 64, 0, 96, 41, 0)]))])
    add("msg_sz0", [(ED, b"", g.self_ix([0]))])
    add("msg_sz0_at_end", [(OTHER, b"", holder), (ED, b"", table([record(0, 0, 64, 0, len(holder), 0, 0)]))])
    add("msg_sz0_past_end", [(OTHER, b"", holder), (ED, b"", table([record(0, 0, 64, 0, len(holder) + 1, 0, 0)]))])
    add("msg_sz_ffff", [(OTHER, b"", holder), (ED, b"", table([record(0, 0, 64, 0, 0, 0xFFFF, 0)]))])
    # aliasing: records that share signature, key and message; and a table that is its own signature's bytes
    add("alias", [(OTHER, b"", holder), (ED, b"", table([hrec()] * 5))])
    add("alias_table_bytes", [(ED, b"", table([record(0, 0xFFFF, 2, 0xFFFF, 0, 0, 0xFFFF)] * 5))])
    # order within one instruction
    add("order_badsig_then_badoff", [(ED, b"", _patch(g.self_ix([10, 10], ["S", None]), 1, 0, 0xFFF0))])
    add("order_good_badoff_badsig", [(ED, b"", _patch(g.self_ix([10, 10, 10], [None, None, "S"]), 1, 2, 0xFFF0))])
    # order across two Ed25519 instructions
    add("order_sig_then_size", [(ED, b"", g.self_ix([10], ["R"])), (ED, b"", b"\1")])
    add("order_good_then_size", [(ED, b"", g.self_ix([10])), (OTHER, b"", b"q"), (ED, b"", b"\1")])
    add("order_size_then_more_ed", [(ED, b"", b"\1"), (ED, b"", g.self_ix([10], ["S"])), (ED, b"", b"\0\0")])
    add("order_off_then_good", [(ED, b"", _patch(g.self_ix([10, 10]), 0, 4, 0xFFF0)), (ED, b"", g.self_ix([10]))])
    # other programs
    add("secp_ignored", [(SECP, b"", b"\1" + bytes(10)), (ED, b"", g.self_ix([12]))])
    add("secp_only", [(SECP, b"", b"\1" + bytes(10))])
    accts = [g.payer] + [g.rng.bytes(32) for _ in range(9)] + [ED25519_ID]
    add("id_last_account", [(10, b"\1\2", g.self_ix([30])), (9, b"", g.self_ix([30], ["S"]))], accts=accts)
    near = ED25519_ID[:31] + b"\1"
    add("id_near_miss", [(1, b"", b"\1")], accts=[g.payer, near])
    # ed_code of each failure kind
    for bad in ("S", "key", "R", "msg"):
        add(f"bad_{bad}", [(ED, b"", g.self_ix([50, 50, 50], [None, bad, None]))])
    # message lengths around the SHA-512 block boundaries (R | A | M: 64 + len), many records, v0
    add("lens_a", [(ED, b"", g.self_ix([0, 1, 47, 48, 63]))])
    add("lens_b", [(ED, b"", g.self_ix([64, 65, 111, 112]))])
    add("long_msg", [(ED, b"", g.self_ix([880]))])
    add("records_8", [(ED, b"", g.self_ix([1] * 8, [None] * 7 + ["R"]))])
    add("v0", [(ED, b"", g.self_ix([70]))], v0=True)
    add("v0_lut", [(ED, b"\4", g.self_ix([70], ["S"]))], v0=True, luts=[(g.rng.bytes(32), b"\1", b"")])
    # the size bound: one instruction of as many shared records as fit
    out.append(max_records(g, MTU))
    out.append(max_records(g, 400))
    # payloads that do not parse
    good = next(c for c in out if c.name == "self_ffff").payload
    out.append(Case("parse_trailing", good + b"\0", None))
    out.append(Case("parse_truncated", good[:-1], None))
    out.append(Case("parse_empty", b"", None))
    out.append(Case("parse_sig_cnt0", b"\0" + good[1:], None))
    return out


def _patch(data, rec, field, value):
    """record rec's u16 field of an instruction's data set to value"""
    b = bytearray(data)
    struct.pack_into("<H", b, 2 + 14 * rec + 2 * field, value)
    return bytes(b)


def max_records(g, sz):
    """A transaction of exactly sz bytes with one Ed25519 instruction of as
    many records as fit, all naming the table's own bytes as signature and key
    and an empty message: two accounts, so nothing smaller carries them."""
    n = sig_bound(sz)
    accts = [g.payer, ED25519_ID]
    body = 2 + 14 * n
    fill = sz - 166 - 2 - len(cu16(body)) - body
    if fill and len(cu16(body + fill)) != len(cu16(body)):
        fill -= 1
    data = table([record(0, 0xFFFF, 8, 0xFFFF, 0, 0, 0xFFFF)] * n) + bytes(max(fill, 0))
    payload, offs = build_txn(accts, [(1, b"", data)])
    return Case(f"max_records_{sz}", payload, (accts, [(1, b"", data)], offs))


def random_txn(g, n_rec, msg_len=8, bad_at=None):
    """One transaction with n_rec <= 64 records (0: no Ed25519 instruction)
    that share the signature, key and message of a holder instruction; record
    bad_at takes its signature one byte further on, which verifies as
    nothing."""
    accts = [g.payer, g.other, ED25519_ID]
    if n_rec == 0:
        return g.case("r0", [(1, b"", g.rng.bytes(1 + g.rng.below(40)))], accts=accts)
    s, p, m = g.triple(msg_len)
    recs = [record(0, 0, 64, 0, 96, msg_len, 0)] * n_rec
    if bad_at is not None:
        recs[bad_at % n_rec] = record(1, 0, 64, 0, 96, msg_len, 0)
    return g.case(f"r{n_rec}", [(1, b"", s + p + m), (2, b"", table(recs))], accts=accts)


def expected(cases, verify):
    """-> (codes int8[n], info tuples, recs lists)"""
    r = [verdict(c.payload, c.model, verify) for c in cases]
    return np.array([x[0] for x in r], dtype=np.int8), [x[1] for x in r], [x[2] for x in r]
