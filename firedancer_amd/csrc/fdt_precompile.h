/* fdt_precompile.h -- the Ed25519 precompile's rules as one source for the
   host and the GPU: which instructions of a parsed transaction are Ed25519
   instructions, how their record tables resolve to (signature, key, message)
   triples, and how the records' verify codes give the transaction's verdict.

   Restates, in the reference's order,
     fd_executor_verify_precompiles  src/flamenco/runtime/fd_executor.c:252-270
     fd_precompile_get_instr_data    src/flamenco/runtime/program/fd_precompiles.c:73-111
     fd_precompile_ed25519_verify    fd_precompiles.c:117-206
   The reference stops at the first failing event in (instruction, record)
   order, where a record's event is its offsets failure or, failing that, its
   verify failure.  Here that is two functions:
     fdt_precompile_walk_core     visits the records in order, emits each one
                                  that resolves, and stops emitting at the
                                  first structural failure (data size, data
                                  offsets), which it reports with its position;
     fdt_precompile_verdict_core  takes the fd_ed25519 codes of the emitted
                                  records in order: the first non-zero one is
                                  the verdict (it lies before the structural
                                  failure), else the structural failure, else 0.
   Records behind a structural failure are never emitted, so verifying every
   emitted record rather than stopping at the first bad one changes nothing.
   The secp256k1 precompile is not restated here: its instructions are
   skipped like those of any other program.  Its rules are fdt_secp256k1.h's
   (include/fd_secp256k1_gpu.h), which reuses this file's reader, walk record
   and verdict rule.

   Compiled by g++ into libfd_verify_tile.so (fdt_precompile_walk,
   fdt_precompile_verdict) and by hipcc into fdgpu_precompile_ingest_kernel /
   fdgpu_precompile_finish_kernel (one transaction per lane).

   Bounds: the input is a payload and the fdt_txn_t fdt_parse_core made of
   that payload, so instr_cnt <= FDT_TXN_INSTR_MAX, every program_id <
   acct_addr_cnt with the account addresses inside the payload, and every
   instruction's [data_off, data_off + data_sz) inside it.  Every read below
   is of an account address or of instruction data at an offset checked
   against data_sz first; both loops are bounded (64 instructions, 255
   records).  On the GPU the reads go through 16-B windows like fdt_reader's,
   which may touch the arena's slack behind the payload; what they hold there
   never reaches a decision. */
#pragma once

#include <stdint.h>

#include "fdt_parse.h"

/* Ed25519SigVerify111111111111111111111111111 (fd_precompiles.c's caller
   compares fd_solana_ed25519_sig_verify_program_id, fd_executor.c:259), as
   little-endian words of its 32 bytes 037d46d6 7c93fbbe 12f9428f 838d40ff
   05707449 27f48a64 fcca7044 80000000 */
FDT_HD uint32_t fdt_precompile_ed25519_id_word(uint32_t w) {
  return w == 0u ? 0xd6467d03u : w == 1u ? 0xbefb937cu : w == 2u ? 0x8f42f912u : w == 3u ? 0xff408d83u :
         w == 4u ? 0x49747005u : w == 5u ? 0x648af427u : w == 6u ? 0x4470cafcu : 0x00000080u;
}

/* The walk's reader: at(k) is payload byte k, k inside the payload (the
   callers check).  A plain load on the host.  On the GPU, as fdt_reader does
   and for its reasons, the aligned 16 B around the last byte read stay in
   registers and are reloaded only when a read leaves them (the arena has
   FDGPU_ARENA_SLACK readable bytes past its end).  The window is two 64-bit
   halves, both read before the choice between them, so that the compiler
   keeps the reader in registers (a choice between the members themselves
   becomes an indexed load, and the struct then lives in memory). */
struct fdt_precompile_reader {
  const uint8_t *p;
#if defined(__HIP_DEVICE_COMPILE__)
  const uint8_t *wb = nullptr;           /* 16-B aligned address of the window */
  uint64_t lo = 0, hi = 0;
  __device__ __forceinline__ uint32_t at(uint64_t k) {
    const uint8_t *a = p + k;
    const uint32_t o = (uint32_t)((uintptr_t)a & 15u);
    const uint8_t *b = a - o;
    uint64_t l = lo, h = hi;
    if (b != wb) {
      const uint4 v = *(const uint4 *)b;
      l = (uint64_t)v.x | ((uint64_t)v.y << 32); h = (uint64_t)v.z | ((uint64_t)v.w << 32);
      lo = l; hi = h; wb = b;
    }
    const uint64_t q = (o & 8u) ? h : l;
    return (uint32_t)(q >> ((o & 7u) * 8u)) & 0xFFu;
  }
#else
  FDT_HDM uint32_t at(uint64_t k) { return p[k]; }
#endif
};

#define FDT_PRECOMPILE_DATA_START    16u   /* DATA_START: 2 + one record (fd_precompiles.c:133) */
#define FDT_PRECOMPILE_OFFSETS_START  2u   /* SIGNATURE_OFFSETS_START */
#define FDT_PRECOMPILE_OFFSETS_SZ    14u   /* SIGNATURE_OFFSETS_SERIALIZED_SIZE: seven u16 */
#define FDT_PRECOMPILE_NONE      0xFFFFu   /* no position; as an instruction index: the current one (:88) */

/* The most records a transaction of sz bytes can emit.  The smallest
   transaction with an instruction is 166 bytes: the signature count (1), one
   signature (64), the legacy header (3), the account count (1), two account
   addresses -- the fee payer and a program, which may not be the fee payer
   (64) --, the blockhash (32) and the instruction count (1).  An Ed25519
   instruction with c records adds at least 5 + 14 c: program index, an empty
   account list, the data size (one byte or more), the table's two leading
   bytes and the records.  What a record points to costs nothing more: its
   signature, key and message may lie in the table itself, and records may
   share them.  So k >= 1 such instructions with R records in all take at
   least 166 + 5 k + 14 R >= 171 + 14 R bytes, and R <= (sz - 171) / 14, which
   is 75 at FDT_TXN_MTU. */
FDT_HD uint32_t fdt_precompile_sig_bound(uint64_t sz) {
  const uint64_t s = sz < FDT_TXN_MTU ? sz : FDT_TXN_MTU;
  return s >= 171u + FDT_PRECOMPILE_OFFSETS_SZ ? (uint32_t)((s - 171u) / FDT_PRECOMPILE_OFFSETS_SZ) : 0u;
}

/* Is the program of instruction `ins` the Ed25519 precompile (fd_executor.c:
   256-259)?  program_id < acct_addr_cnt (fdt_parse_core), so the 32 bytes lie
   inside the payload. */
FDT_HD bool fdt_precompile_is_ed25519(fdt_precompile_reader &r, const fdt_txn_t *t, const fdt_txn_instr_t &ins) {
  const uint64_t a = (uint64_t)t->acct_addr_off + 32u * ins.program_id;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (uint32_t w = 0; w < 8u; w++) {
    const uint32_t v = r.at(a + 4u * w) | (r.at(a + 4u * w + 1u) << 8) | (r.at(a + 4u * w + 2u) << 16) |
                       (r.at(a + 4u * w + 3u) << 24);
    if (v != fdt_precompile_ed25519_id_word(w)) return false;
  }
  return true;
}

/* a little-endian u16 at an unaligned payload offset */
FDT_HD uint32_t fdt_precompile_u16(fdt_precompile_reader &r, uint64_t k) { return r.at(k) | (r.at(k + 1u) << 8); }

/* fd_precompile_get_instr_data (fd_precompiles.c:73-111): `size` bytes at
   `off` of instruction idx's data -- 0xFFFF: the current one, cur (:88); any
   other index must name an instruction (:97), of any program, earlier or
   later -- lie inside that data (:106).  *at: their payload offset. */
FDT_HD bool fdt_precompile_resolve(const fdt_txn_t *t, uint32_t cur, uint32_t idx, uint32_t off, uint32_t size,
                                   uint32_t *at) {
  const uint32_t k = idx == FDT_PRECOMPILE_NONE ? cur : idx;
  if (k >= t->instr_cnt) return false;
  if (off + size > t->instr[k].data_sz) return false;       /* off + size < 2^17 */
  *at = (uint32_t)t->instr[k].data_off + off;
  return true;
}

/* The walk.  emit(instr_idx, rec_idx, sig_off, pub_off, msg_off, msg_sz)
   (payload offsets) is called for each record that resolves, in order, until
   the first structural failure; out->rec_cnt counts the calls.  out->code is
   0, FDGPU_CODE_PRECOMPILE_DATA_SIZE at (instruction, 0xFFFF) or
   FDGPU_CODE_PRECOMPILE_DATA_OFFSET at (instruction, record); the Ed25519
   instructions are counted through the whole transaction, past a failure
   too. */
template <class Emit>
FDT_HD void fdt_precompile_walk_core(const uint8_t *payload, uint64_t payload_sz, const fdt_txn_t *t, Emit &emit,
                                     fdt_precompile_walk_t *out) {
  fdt_precompile_reader r;
  r.p = payload;
  (void)payload_sz;
  int32_t code = 0;
  uint32_t f_instr = FDT_PRECOMPILE_NONE, f_rec = FDT_PRECOMPILE_NONE, ed_cnt = 0, rec_cnt = 0;
  const uint32_t instr_cnt = t->instr_cnt <= FDT_TXN_INSTR_MAX ? t->instr_cnt : (uint32_t)FDT_TXN_INSTR_MAX;
  for (uint32_t j = 0; j < instr_cnt; j++) {                 /* fd_executor.c:255 */
    const fdt_txn_instr_t ins = t->instr[j];
    if (!fdt_precompile_is_ed25519(r, t, ins)) continue;
    ed_cnt++;
    if (code) continue;                                      /* the reference has returned (fd_executor.c:260-262) */
    const uint32_t data_off = ins.data_off, data_sz = ins.data_sz;
    if (data_sz < FDT_PRECOMPILE_DATA_START) {               /* :133-138; data[0] is read only when data_sz == 2 */
      if (data_sz == 2u && r.at(data_off) == 0) continue;
      code = FDGPU_CODE_PRECOMPILE_DATA_SIZE; f_instr = j;
      continue;
    }
    const uint32_t cnt = r.at(data_off);                     /* :140; data[1] is padding, never read */
    if (cnt == 0u || data_sz < cnt * FDT_PRECOMPILE_OFFSETS_SZ + FDT_PRECOMPILE_OFFSETS_START) {   /* :141-149 */
      code = FDGPU_CODE_PRECOMPILE_DATA_SIZE; f_instr = j;
      continue;
    }
    for (uint32_t i = 0; i < cnt; i++) {                     /* :152; cnt <= 255 */
      const uint64_t b = (uint64_t)data_off + FDT_PRECOMPILE_OFFSETS_START + FDT_PRECOMPILE_OFFSETS_SZ * i;
      /* fd_ed25519_signature_offsets_t (fd_precompiles.c:23,153): seven packed little-endian u16 */
      const uint32_t sig_offset = fdt_precompile_u16(r, b), sig_instr = fdt_precompile_u16(r, b + 2u),
                     pub_offset = fdt_precompile_u16(r, b + 4u), pub_instr = fdt_precompile_u16(r, b + 6u),
                     msg_offset = fdt_precompile_u16(r, b + 8u), msg_sz = fdt_precompile_u16(r, b + 10u),
                     msg_instr = fdt_precompile_u16(r, b + 12u);
      uint32_t sig_at = 0, pub_at = 0, msg_at = 0;
      if (!fdt_precompile_resolve(t, j, sig_instr, sig_offset, 64u, &sig_at) ||       /* :161-167 */
          !fdt_precompile_resolve(t, j, pub_instr, pub_offset, 32u, &pub_at) ||       /* :175-181 */
          !fdt_precompile_resolve(t, j, msg_instr, msg_offset, msg_sz, &msg_at)) {    /* :190-196 */
        code = FDGPU_CODE_PRECOMPILE_DATA_OFFSET; f_instr = j; f_rec = i;
        break;
      }
      emit(j, i, sig_at, pub_at, msg_at, msg_sz);            /* :201: one fd_ed25519_verify */
      rec_cnt++;
    }
  }
  out->code = code;
  out->rec_cnt = rec_cnt;
  out->instr_idx = (uint16_t)f_instr;
  out->rec_idx = (uint16_t)f_rec;
  out->ed_instr_cnt = (uint16_t)ed_cnt;
  out->_pad = 0;
}

/* The verdict of a walk whose n = rec_cnt records were all verified:
   code_at(k) is record k's fd_ed25519 code, pos_at(k) its instr_idx << 16 |
   rec_idx.  The first failed verify gives SIGNATURE at its position with its
   code kept (:201-202: every emitted record lies before the structural
   failure), else the structural failure, else 0. */
template <class CodeAt, class PosAt>
FDT_HD int fdt_precompile_verdict_core(int32_t walk_code, uint32_t f_instr, uint32_t f_rec, uint32_t ed_instr_cnt,
                                       uint32_t n, CodeAt code_at, PosAt pos_at, fdgpu_precompile_info_t *info) {
  int32_t code = walk_code, ed = 0;
  for (uint32_t k = 0; k < n; k++) {
    const int c = code_at(k);
    if (c) {
      const uint32_t p = pos_at(k);
      code = FDGPU_CODE_PRECOMPILE_SIGNATURE; ed = c; f_instr = p >> 16; f_rec = p & 0xFFFFu;
      break;
    }
  }
  info->instr_idx = (uint16_t)f_instr;
  info->rec_idx = (uint16_t)f_rec;
  info->ed_instr_cnt = (uint16_t)ed_instr_cnt;
  info->sig_cnt = (uint16_t)n;
  info->ed_code = (int8_t)ed;
  for (int k = 0; k < 7; k++) info->_pad[k] = 0;
  return code;
}

/* the info of a transaction nothing was run for (PARSE_FAIL, CAP) */
FDT_HD void fdt_precompile_info_none(fdgpu_precompile_info_t *info) {
  info->instr_idx = (uint16_t)FDT_PRECOMPILE_NONE;
  info->rec_idx = (uint16_t)FDT_PRECOMPILE_NONE;
  info->ed_instr_cnt = 0;
  info->sig_cnt = 0;
  info->ed_code = 0;
  for (int k = 0; k < 7; k++) info->_pad[k] = 0;
}
