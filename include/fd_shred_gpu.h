/* fd_shred_gpu.h -- raw Merkle shreds to verdicts on the GPU engine.

   What the shred tile does to the first shred of each FEC set before it
   trusts it (fd_fec_resolver_add_shred, src/disco/shred/fd_fec_resolver.c:
   333-443): parse and header checks, the SHA-256 Merkle leaf over the
   shred's ~1.1 KB, the walk up its 20-byte inclusion proof to the root, and
   fd_ed25519_verify(root, 32, signature, leader).  Here all of it runs on
   the device: the packets go up as one arena, the codes and the roots come
   back.  The rules are those of firedancer_amd/csrc/fdt_shred.h (the one
   source the host library libfd_verify_tile.so also compiles, as
   fdt_shred_check / fdt_shred_root).

   An extension of fd_ed25519_gpu.h: same engine, same ring slots, tickets
   and error codes.  Exported from libfd_ed25519_gpu.so.  Plain C11. */
#ifndef FD_SHRED_GPU_H
#define FD_SHRED_GPU_H

#include <stddef.h>
#include <stdint.h>

#include "fd_ed25519_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* shred = arena[off, off+sz); its leader's public key at arena[pub_off, +32) */
typedef struct {
  uint32_t off;
  uint32_t sz;
  uint32_t pub_off;
} fdgpu_shred_t;

/* the shred failed a check before the signature (the tile drops it
   unverified); its root is reported as zeros */
#define FDGPU_CODE_SHRED_REJECT (-67)
/* bytes of a shred the engine accepts: FD_SHRED_MAX_SZ and a little trailing
   data, which the parser tolerates (fd_shred.c:46-54) */
#define FDGPU_SHRED_SZ_MAX (1228u + 4u)

/* A ring batch of n shreds, with fdgpu_submit_frags' slot semantics: an arena
   inside a fdgpu_host_register'ed region is uploaded in place by DMA (and
   must stay unchanged until the poll), any other is staged.  Returns the
   ticket, FDGPU_ERR_FULL, or FDGPU_ERR_INVAL when n exceeds the engine's
   max_txn or max_sig, a shred or key lies outside the arena, a shred is
   larger than FDGPU_SHRED_SZ_MAX, or the arena, its slack (160 B) and the
   32 n bytes of roots do not fit max_arena.  n == 0 is a valid empty batch. */
int64_t fdgpu_submit_shreds( fdgpu_engine_t * e, uint8_t const * arena, uint64_t arena_sz,
                             fdgpu_shred_t const * shreds, uint64_t n, uint16_t expected_version );

/* codes[i]: what fd_ed25519_verify(root_i, 32, shred_i, leader_i) returns (0,
   -1, -2, -3), or FDGPU_CODE_SHRED_REJECT; roots (NULL: not wanted): 32 n
   bytes.  Returns FDGPU_OK, FDGPU_PENDING (non-blocking) or an error. */
int fdgpu_poll_shreds( fdgpu_engine_t * e, int64_t ticket, int8_t * codes, uint8_t * roots, int blocking );

/* Diagnostics: synchronous, host pointers, outside the ring. */
/* SHA-256 of arena[msg_off, +msg_sz) per record (the other fields unused): out 32 n bytes */
int fdgpu_debug_sha256( fdgpu_engine_t * e, uint8_t const * arena, uint64_t arena_sz, fdgpu_txn_t const * msgs,
                        uint64_t n, uint8_t * out );
/* the checks and the roots alone: ok[i] = 0 or FDGPU_CODE_SHRED_REJECT */
int fdgpu_debug_shred_roots( fdgpu_engine_t * e, uint8_t const * arena, uint64_t arena_sz,
                             fdgpu_shred_t const * shreds, uint64_t n, uint16_t expected_version, int8_t * ok,
                             uint8_t * roots );
/* the batch resident on the device: the mean time of its ingest (checks,
   hashes, records) and of its verify over iters runs each, in ms */
int fdgpu_debug_shred_time( fdgpu_engine_t * e, uint8_t const * arena, uint64_t arena_sz,
                            fdgpu_shred_t const * shreds, uint64_t n, uint16_t expected_version, int iters,
                            double * ingest_ms, double * verify_ms );

#ifdef __cplusplus
}
#endif

#endif /* FD_SHRED_GPU_H */
