/* fd_shred_sets_gpu.h -- every shred of a batch to a verdict on the GPU engine:
   one signature verified per FEC set, shreds of known sets held against the
   root the caller already trusts.

   The shred tile receives all shreds of an FEC set (64 at the usual 32:32).
   For the first it does what fd_shred_gpu.h does; for every later one
   (fd_fec_resolver_add_shred, src/disco/shred/fd_fec_resolver.c:466-484) it
   checks no signature: it hashes the leaf and holds the proof against the tree
   the first shred opened.  A set batch takes any received shreds and gives
   each its code and its root with one verify lane per distinct (signature,
   root, leader key) in the batch, and none for a shred whose set's root the
   caller names.  The resolver's map of open sets, its duplicate and variant
   checks, Reed-Solomon and resigning stay with the caller.

   The rule per shred i, in this order:
     1. the checks of firedancer_amd/csrc/fdt_shred.h fail: code
        FDGPU_CODE_SHRED_REJECT, root zeros, rep UINT32_MAX (as
        fdgpu_submit_shreds);
     2. known_off is set: code 0 when the derived root equals the 32 bytes at
        known_off, else FDGPU_CODE_SHRED_ROOT_MISMATCH; the derived root is
        reported either way, no verify lane is used, rep UINT32_MAX;
     3. otherwise the shred's key is its 128 bytes (signature 64, derived root
        32, leader key 32): code = fd_ed25519_verify(root, 32, signature,
        leader), computed once per distinct key of the batch; rep = the index
        of the shred whose lane computed it (rep[i] == i: shred i ran).  Any
        shred of a group may be its representative: the code is a function of
        the key only.  A group whose shreds the bounded table search does not
        bring together (more than 32 keys that share the signature's first
        half and the root) is verified more than once, with the same codes.

   An extension of fd_shred_gpu.h: same engine, ring slots, tickets and error
   codes.  Exported from libfd_ed25519_gpu.so.  Plain C11. */
#ifndef FD_SHRED_SETS_GPU_H
#define FD_SHRED_SETS_GPU_H

#include <stddef.h>
#include <stdint.h>

#include "fd_shred_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FDGPU_SHRED_NO_ROOT 0xffffffffu

/* shred = arena[off, off+sz); its leader's public key at arena[pub_off, +32);
   known_off: FDGPU_SHRED_NO_ROOT, or arena[known_off, +32) = the root of this
   shred's set as the caller already trusts it */
typedef struct {
  uint32_t off;
  uint32_t sz;
  uint32_t pub_off;
  uint32_t known_off;
} fdgpu_set_shred_t;

/* the shred passed its checks, but its derived root is not the known one */
#define FDGPU_CODE_SHRED_ROOT_MISMATCH (-74)

/* A ring batch of n shreds with fdgpu_submit_shreds' arguments, slot
   semantics, registered-arena DMA and roots region behind the arena's slack.
   Returns the ticket, FDGPU_ERR_FULL, or FDGPU_ERR_INVAL for what
   fdgpu_submit_shreds rejects and for a known_off + 32 > arena_sz.  n == 0 is
   a valid empty batch. */
int64_t fdgpu_submit_shred_sets( fdgpu_engine_t * e, uint8_t const * arena, uint64_t arena_sz,
                                 fdgpu_set_shred_t const * shreds, uint64_t n, uint16_t expected_version );

/* codes[i], roots (32 n bytes) and rep[i] by the rule above; *lanes = the
   verify lanes the batch used.  roots, rep and lanes may be NULL.  Returns
   FDGPU_OK, FDGPU_PENDING (non-blocking) or an error. */
int fdgpu_poll_shred_sets( fdgpu_engine_t * e, int64_t ticket, int8_t * codes, uint8_t * roots, uint32_t * rep,
                           uint64_t * lanes, int blocking );

/* Diagnostic (synchronous, host pointers, outside the ring): the batch
   resident on the device, the mean time of its ingest and dedup and of its
   verify over iters runs each, in ms */
int fdgpu_debug_shred_sets_time( fdgpu_engine_t * e, uint8_t const * arena, uint64_t arena_sz,
                                 fdgpu_set_shred_t const * shreds, uint64_t n, uint16_t expected_version, int iters,
                                 double * ingest_ms, double * verify_ms );

#ifdef __cplusplus
}
#endif

#endif /* FD_SHRED_SETS_GPU_H */
