/* fd_poh_gpu.h -- a block's proof of history on the GPU engine.

   The half of the replay block check that is not signatures: what
   fd_runtime_block_verify_tpool (src/flamenco/runtime/fd_runtime.c:2274-2371)
   does for every microblock ("entry") before it trusts a block.  It hashes
   the previous entry's hash forward hash_cnt times (fd_poh_append), builds
   the 32-byte Merkle root of the entry's signatures (fd_wbmtree32: hash 32 B,
   prefix 1 B), mixes the root in (fd_poh_mixin) and compares the result with
   the hash the entry claims.  Here the leaves, the roots and the chains run
   on the device; the codes and the computed hashes come back.

   The work is sequential inside an entry and independent across entries
   (every entry starts from its predecessor's *claimed* hash), so the device
   runs one chain per lane.  That pays for bulk work -- many entries of many
   blocks in one batch -- and not for the latency of one block: a lone chain
   on one lane is far slower than on a host core (profiles/poh/README.md).

   An extension of fd_ed25519_gpu.h: same engine, same ring slots, tickets
   and error codes.  Exported from libfd_ed25519_gpu.so.  Plain C11. */
#ifndef FD_POH_GPU_H
#define FD_POH_GPU_H

#include <stddef.h>
#include <stdint.h>

#include "fd_ed25519_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FDGPU_POH_NO_MIX        0xFFFFFFFFu
#define FDGPU_POH_HASH_CNT_MAX  (1u<<20)   /* per entry, hard ceiling: bounds a launch's duration */
#define FDGPU_CODE_POH_MISMATCH (-68)      /* the computed hash is not the claimed one */
#define FDGPU_CODE_POH_TOO_LONG (-69)      /* hash_cnt above the batch's cap: not run, hash reported as zeros */

typedef struct {
  uint64_t hash_cnt;
  uint32_t prev_off;   /* arena[prev_off,+32): the hash the entry starts from   */
  uint32_t hash_off;   /* arena[hash_off,+32): the hash the entry claims        */
  uint32_t sig_first;  /* its signatures: sig_offs[sig_first, +sig_cnt), each   */
  uint32_t sig_cnt;    /*   the arena offset of 64 bytes; 0: no transactions    */
  uint32_t mix_off;    /* FDGPU_POH_NO_MIX, or arena[mix_off,+32) mixed in as   */
  uint32_t _pad;       /*   given (then sig_cnt must be 0)                      */
} fdgpu_poh_entry_t;   /* 32 bytes */

/* Per entry (fd_runtime_poh_verify_wide_task):
     no signatures and no mix   out = append(prev, hash_cnt)
     otherwise                  out = mixin(append(prev, hash_cnt ? hash_cnt-1 : 0), root or mix)
   append(h, k) is SHA-256 applied k times to the 32 bytes; mixin(h, m) is
   SHA-256(h || m); root is the Merkle root of the entry's signatures: a leaf
   is SHA-256(0x00 || sig[64]), a branch SHA-256(0x01 || l[32] || r[32]), a
   layer with an odd node count pairs its last node with itself, one leaf is
   its own root.  No alignment is required of any offset.

   hash_cnt comes from untrusted block bytes, so the batch carries a cap
   (1 .. FDGPU_POH_HASH_CNT_MAX; the cluster's hashes per tick): an entry
   above it is never started, its code is FDGPU_CODE_POH_TOO_LONG and its
   hash zeros.

   A ring batch of n entries, with fdgpu_submit_shreds' slot semantics: an
   arena inside a fdgpu_host_register'ed region is uploaded in place by DMA
   (and must stay unchanged until the poll), any other is staged.  Returns the
   ticket, FDGPU_ERR_FULL, or FDGPU_ERR_INVAL when n exceeds the engine's
   max_txn or sig_total its max_sig, a 32- or 64-byte range lies outside the
   arena, an entry's signatures lie outside sig_offs, the entries' signature
   ranges are not ascending and disjoint in entry order (each range is folded
   in place on the device, so no two entries may share a part of sig_offs: an
   entry given twice brings its offsets twice), mix_off is set together with
   sig_cnt, the cap is out of range or the arena exceeds max_arena.
   n == 0 is a valid empty batch. */
int64_t fdgpu_submit_poh( fdgpu_engine_t * e, uint8_t const * arena, uint64_t arena_sz,
                          fdgpu_poh_entry_t const * entries, uint64_t n,
                          uint32_t const * sig_offs, uint64_t sig_total, uint64_t hash_cnt_cap );

/* codes[i]: 0, FDGPU_CODE_POH_MISMATCH or FDGPU_CODE_POH_TOO_LONG; hashes
   (NULL: not wanted): 32 n bytes, every computed out.  Returns FDGPU_OK,
   FDGPU_PENDING (non-blocking) or an error. */
int fdgpu_poll_poh( fdgpu_engine_t * e, int64_t ticket, int8_t * codes, uint8_t * hashes, int blocking );

/* what one PoH batch of this engine may hold (its max_txn entries, max_sig
   signatures, max_arena bytes): a caller that cuts a stream into batches
   asks here.  Any pointer may be NULL.  Returns FDGPU_OK or FDGPU_ERR_INVAL. */
int fdgpu_poh_limits( fdgpu_engine_t * e, uint64_t * entry_max, uint64_t * sig_max, uint64_t * arena_max );

/* Diagnostics: synchronous, host pointers, outside the ring. */
/* hashes a lane runs between two looks at the entry queue (the chain
   kernel's CHUNK: the lengths around it are where its paths change) */
uint32_t fdgpu_poh_chunk( void );
/* the batch's pipeline with the chain kernel's grid forced to grid_waves
   waves (0: the default): few waves make few entries reach the refill path */
int fdgpu_debug_poh( fdgpu_engine_t * e, uint8_t const * arena, uint64_t arena_sz,
                     fdgpu_poh_entry_t const * entries, uint64_t n, uint32_t const * sig_offs, uint64_t sig_total,
                     uint64_t hash_cnt_cap, uint32_t grid_waves, int8_t * codes, uint8_t * hashes );
/* the batch resident on the device: the mean time of its tree (leaves and
   roots) and of its chains over iters runs each, in ms */
int fdgpu_debug_poh_time( fdgpu_engine_t * e, uint8_t const * arena, uint64_t arena_sz,
                          fdgpu_poh_entry_t const * entries, uint64_t n, uint32_t const * sig_offs,
                          uint64_t sig_total, uint64_t hash_cnt_cap, int iters, double * tree_ms, double * chain_ms );

#ifdef __cplusplus
}
#endif

#endif /* FD_POH_GPU_H */
