/* fdgpu_shred.h -- the shred kernels' launchers (fdgpu_shred.hip), shared with
   the host unit that drives them (fdgpu_shreds.cpp).  Not part of the public
   C ABI (that is include/fd_shred_gpu.h). */
#pragma once

#include "../../include/fd_shred_gpu.h"
#include "../../include/fd_shred_sets_gpu.h"
#include "fdgpu_internal.h"

#ifdef __cplusplus
extern "C" {
#endif

/* All asynchronous on `stream`.

   Ingest: shred i of d_shreds (one per lane) through fdt_shred_check and, if
   it passes, the SHA-256 leaf and proof walk; its root goes to d_arena +
   roots_off + 32 i (16-B aligned; inside the arena's allocation, so that the
   verify's 32-bit offsets reach it, with FDGPU_ARENA_SLACK readable bytes
   behind the last root) and it takes the next signature descriptor {msg = its
   root, 32 B, sig = the shred's first 64 bytes, pub = its leader key}: each
   wave claims its passing lanes' descriptor slots with one atomic add on
   *d_n_sig, which must be zero at the start, so a rejected shred costs no
   verify lane.  d_tds[i] = {its descriptor, 1}, or {0, 0} when rejected.  The
   verify then runs from d_sigs and *d_n_sig as for any batch whose signature
   count is produced on the device (fdgpu_launch_verify_sigs). */
hipError_t fdgpu_launch_shred_ingest(uint8_t *d_arena, const fdgpu_shred_t *d_shreds, uint32_t n,
                                     uint16_t expected_version, uint32_t roots_off, fdgpu_sig_desc_t *d_sigs,
                                     fdgpu_txn_desc_t *d_tds, uint32_t *d_n_sig, hipStream_t stream);
/* Finish: d_codes[i] = the code of shred i's signature (the single-signature
   combine; d_sig_codes NULL: 0), or FDGPU_CODE_SHRED_REJECT; d_roots_out + 32 i
   (16-B aligned) = its root, zeros when rejected. */
hipError_t fdgpu_launch_shred_finish(const fdgpu_txn_desc_t *d_tds, uint32_t n, const int8_t *d_sig_codes,
                                     const uint8_t *d_roots, int8_t *d_codes, uint8_t *d_roots_out,
                                     hipStream_t stream);
/* Set batches (include/fd_shred_sets_gpu.h).
   Set ingest: shred i through the checks, the leaf and the proof walk as above, its root to d_arena + roots_off + 32 i;
   d_state[i] = 0 rejected, 1 its root equals the 32 bytes at known_off, 2 it does not, 3 a candidate for a verify lane
   (no known root).
   Set dedup: d_ht, ht_slots (a power of two >= 2 n) words all 0xffffffff at the start, is the table of candidate
   indices keyed by (signature, root, leader key); d_rep_of[i] = the shred that represents candidate i's key (itself
   after 32 probes), 0xffffffff for any other shred; each representative takes the next signature descriptor {msg = its
   root, 32 B, sig = the shred, pub = its leader key} -- one atomic add per workgroup on *d_n_sig, which must be zero
   at the start -- and d_slot_of[i] = that descriptor's index.  The verify then runs from d_sigs and *d_n_sig.
   Set finish: d_codes[i] = FDGPU_CODE_SHRED_REJECT, 0, FDGPU_CODE_SHRED_ROOT_MISMATCH or the code of its
   representative's signature; d_roots_out + 32 i (16-B aligned) = its root, zeros when rejected; *d_lanes_out =
   *d_n_sig. */
hipError_t fdgpu_launch_shred_set_ingest(uint8_t *d_arena, const fdgpu_set_shred_t *d_shreds, uint32_t n,
                                         uint16_t expected_version, uint32_t roots_off, uint8_t *d_state,
                                         hipStream_t stream);
hipError_t fdgpu_launch_shred_set_dedup(const uint8_t *d_arena, const fdgpu_set_shred_t *d_shreds, uint32_t n,
                                        uint32_t roots_off, const uint8_t *d_state, uint32_t *d_ht, uint32_t ht_slots,
                                        uint64_t seed, uint32_t *d_rep_of, uint32_t *d_slot_of, fdgpu_sig_desc_t *d_sigs,
                                        uint32_t *d_n_sig, hipStream_t stream);
hipError_t fdgpu_launch_shred_set_finish(const uint8_t *d_state, const uint32_t *d_rep_of, const uint32_t *d_slot_of,
                                         uint32_t n, const int8_t *d_sig_codes, const uint8_t *d_roots,
                                         const uint32_t *d_n_sig, int8_t *d_codes, uint8_t *d_roots_out,
                                         uint32_t *d_lanes_out, hipStream_t stream);
/* SHA-256 of d_arena[msg_off, +msg_sz) per descriptor: d_out 8 u32 each (the digest's bytes) */
hipError_t fdgpu_launch_test_sha256(const uint8_t *d_arena, const fdgpu_sig_desc_t *d_msgs, uint32_t n,
                                    uint32_t *d_out, hipStream_t stream);

#ifdef __cplusplus
}
#endif
