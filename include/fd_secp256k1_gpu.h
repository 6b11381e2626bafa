/* fd_secp256k1_gpu.h -- a block's secp256k1 precompile instructions to
   verdicts on the GPU engine.

   The second program fd_executor_verify_precompiles checks of every
   transaction (src/flamenco/runtime/fd_executor.c:252-270): each instruction
   whose program is KeccakSecp256k11111111111111111111111111111 carries a
   table of 11-byte records whose offsets point into the data of any
   instruction of the same transaction, and each record is one Keccak-256 of
   a message, one ECDSA public-key recovery on secp256k1, one Keccak-256 of
   the recovered key and a compare of its last 20 bytes with an Ethereum
   address (fd_precompile_secp256k1_verify, program/fd_precompiles.c:212-307).
   Here all of it runs on the device, as fd_precompile_gpu.h's batches do for
   Ed25519SigVerify111...: the raw transactions go up as one arena, are parsed
   there, their record tables are walked, every record that resolves becomes
   one lane of the recover kernel, and one code and one info record per
   transaction come back.  The rules are those of
   firedancer_amd/csrc/fdt_secp256k1.h (the one source the host library
   libfd_verify_tile.so also compiles, as fdt_secp256k1_walk /
   fdt_secp256k1_recover / fdt_secp256k1_verdict).

   A batch of this kind looks at secp256k1 instructions only; the Ed25519
   ones are fdgpu_submit_precompiles', and fd_verify_tile.h's
   fdgpu_precompile_merge joins the two verdicts.  The one feature gate the
   reference consults, libsecp256k1_fail_on_bad_count, is a flag the caller
   states.

   An extension of fd_precompile_gpu.h: same engine, same ring slots, tickets,
   error codes, transaction records (fdgpu_precompile_t), info records and
   FDGPU_CODE_PRECOMPILE_* codes.  Exported from libfd_ed25519_gpu.so.
   Plain C11. */
#ifndef FD_SECP256K1_GPU_H
#define FD_SECP256K1_GPU_H

#include <stddef.h>
#include <stdint.h>

#include "fd_precompile_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* flags of a batch */
#define FDGPU_SECP256K1_FAIL_ON_BAD_COUNT 1u  /* libsecp256k1_fail_on_bad_count is active: a table that
                                                 states 0 records in more than one byte of data is DATA_SIZE */

/* A record's code, kept in info.ed_code of a transaction whose code is
   FDGPU_CODE_PRECOMPILE_SIGNATURE because a record's check failed (the
   reference maps all of them to one error): */
#define FDGPU_SECP256K1_ERR_RECID    (-1)  /* recovery id outside 0..3 */
#define FDGPU_SECP256K1_ERR_RANGE    (-2)  /* r or s is 0, or not below the group order */
#define FDGPU_SECP256K1_ERR_POINT    (-3)  /* no curve point has the x the signature names (or r + n >= p) */
#define FDGPU_SECP256K1_ERR_INFINITY (-4)  /* the recovered key is the point at infinity */
#define FDGPU_SECP256K1_ERR_ADDRESS  (-5)  /* the key's address differs from the record's */
/* info.ed_code is 0 where SIGNATURE is a record's bytes leaving their
   instruction's data (the reference returns that error for it, fd_precompiles.c:
   106-108).  In the info record, ed_instr_cnt counts the transaction's
   secp256k1 instructions and sig_cnt the records checked. */

/* The most records a transaction of sz bytes can send to the recover kernel:
   the sig_cap of a caller that has not parsed it (derived at
   fdt_secp256k1_sig_bound, fdt_secp256k1.h). */
uint32_t fdgpu_secp256k1_sig_bound( uint64_t sz );

/* A ring batch of n transactions, with fdgpu_submit_precompiles' slot, error
   and cap semantics (sig_cap: the record slots reserved for the transaction;
   they sum to at most the engine's max_sig).  flags: FDGPU_SECP256K1_*.
   n == 0 is a valid empty batch. */
int64_t fdgpu_submit_secp256k1( fdgpu_engine_t * e, uint8_t const * arena, uint64_t arena_sz,
                                fdgpu_precompile_t const * txns, uint64_t n, uint32_t flags );

/* codes[i]: 0 (every secp256k1 instruction of the transaction passes, or it
   has none), FDGPU_CODE_PRECOMPILE_DATA_SIZE, _DATA_OFFSET, _SIGNATURE or
   _CAP -- the first failing event in (instruction, record) order --, or
   FDGPU_CODE_PARSE_FAIL.  info (NULL: not wanted): n records; on PARSE_FAIL
   and CAP {0xFFFF, 0xFFFF, 0, 0, 0}.  Returns FDGPU_OK, FDGPU_PENDING
   (non-blocking) or an error. */
int fdgpu_poll_secp256k1( fdgpu_engine_t * e, int64_t ticket, int8_t * codes, fdgpu_precompile_info_t * info,
                          int blocking );

/* Diagnostics: synchronous, host pointers, outside the ring. */
/* the ingest alone, as fdgpu_debug_precompile_walk: descs 4 u32 per record
   slot {msg_off, msg_sz, sig_off, addr_off} (arena offsets); in walk,
   ed_instr_cnt counts the secp256k1 instructions and code may also be
   FDGPU_CODE_PRECOMPILE_SIGNATURE (bytes that leave their instruction). */
int fdgpu_debug_secp256k1_walk( fdgpu_engine_t * e, uint8_t const * arena, uint64_t arena_sz,
                                fdgpu_precompile_t const * txns, uint64_t n, uint32_t flags,
                                fdgpu_precompile_walk_t * walk, uint32_t * descs, uint32_t * pos, uint64_t desc_cap,
                                uint64_t * desc_cnt );
/* n messages arena[off_sz[2 i], + off_sz[2 i + 1]), each at most 1232 bytes,
   to n Keccak-256 digests of 32 bytes, one message per lane */
int fdgpu_debug_keccak256( fdgpu_engine_t * e, uint8_t const * arena, uint64_t arena_sz, uint32_t const * off_sz,
                           uint64_t n, uint8_t * digests );
/* n x 97 bytes (hash[32], r[32], s[32], recovery id) to n codes (0 or
   FDGPU_SECP256K1_ERR_RECID .. _INFINITY) and n keys x[32] | y[32] (zeros
   where the code is not 0), one record per lane */
int fdgpu_debug_secp256k1_recover( fdgpu_engine_t * e, uint8_t const * in, uint64_t n, int8_t * codes, uint8_t * keys );
/* the batch resident on the device: the mean time of its ingest (parse, two
   walks, descriptors) and of its recover kernel over iters runs each, in ms */
int fdgpu_debug_secp256k1_time( fdgpu_engine_t * e, uint8_t const * arena, uint64_t arena_sz,
                                fdgpu_precompile_t const * txns, uint64_t n, uint32_t flags, int iters,
                                double * ingest_ms, double * recover_ms );

#ifdef __cplusplus
}
#endif

#endif /* FD_SECP256K1_GPU_H */
