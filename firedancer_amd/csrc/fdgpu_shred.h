/* fdgpu_shred.h -- the shred kernels' launchers (fdgpu_shred.hip), shared with
   the host unit that drives them (fdgpu_shreds.cpp).  Not part of the public
   C ABI (that is include/fd_shred_gpu.h). */
#pragma once

#include "../../include/fd_shred_gpu.h"
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
/* SHA-256 of d_arena[msg_off, +msg_sz) per descriptor: d_out 8 u32 each (the digest's bytes) */
hipError_t fdgpu_launch_test_sha256(const uint8_t *d_arena, const fdgpu_sig_desc_t *d_msgs, uint32_t n,
                                    uint32_t *d_out, hipStream_t stream);

#ifdef __cplusplus
}
#endif
