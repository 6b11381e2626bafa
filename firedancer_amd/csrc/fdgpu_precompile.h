/* fdgpu_precompile.h -- the precompile kernels' launchers
   (fdgpu_precompile.hip), shared with the host unit that drives them
   (fdgpu_precompiles.cpp).  Not part of the public C ABI (that is
   include/fd_precompile_gpu.h). */
#pragma once

#include "../../include/fd_precompile_gpu.h"
#include "fdgpu_internal.h"

#ifdef __cplusplus
extern "C" {
#endif

/* All asynchronous on `stream`.

   Ingest: transaction i of d_txns (one per lane, one wave per block) through
   fdt_parse_core into d_txn_out + 852 i (FD_TXN_MAX_SZ; 2-B aligned) and a
   first fdt_precompile_walk_core that only counts the records that resolve.
   A count above sig_cap is FDGPU_CODE_PRECOMPILE_CAP and counts as none.
   Each wave claims its lanes' signature slots with one inclusive scan of the
   counts and one atomic add on *d_n_sig, which must be zero at the start, so
   a transaction's slots are contiguous and the batch takes at most the sum
   of sig_cap.  A second walk writes d_sigs[slot] (arena offsets) and
   d_pos[slot] = instr_idx << 16 | rec_idx.  d_walk[i] = the slots and the
   walk's structural outcome (fdgpu_precompile_walk_t: 16 B, 16-B aligned).
   The verify then runs from d_sigs and *d_n_sig as for any batch whose
   signature count is produced on the device (fdgpu_launch_verify_sigs). */
hipError_t fdgpu_launch_precompile_ingest(const uint8_t *d_arena, const fdgpu_precompile_t *d_txns, uint32_t n,
                                          uint8_t *d_txn_out, fdgpu_sig_desc_t *d_sigs, uint32_t *d_pos,
                                          fdgpu_precompile_walk_t *d_walk, uint32_t *d_n_sig, hipStream_t stream);
/* Finish: fdt_precompile_verdict_core over transaction i's signature codes
   (d_sig_codes NULL: all 0, the structural outcome alone): d_codes[i] and
   d_info + 16 i (16-B aligned). */
hipError_t fdgpu_launch_precompile_finish(const fdgpu_precompile_walk_t *d_walk, uint32_t n, const int8_t *d_sig_codes,
                                          const uint32_t *d_pos, int8_t *d_codes, uint8_t *d_info,
                                          hipStream_t stream);

#ifdef __cplusplus
}
#endif
