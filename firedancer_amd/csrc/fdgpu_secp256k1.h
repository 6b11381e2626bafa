/* fdgpu_secp256k1.h -- the secp256k1 precompile kernels' launchers
   (fdgpu_secp256k1.hip), shared with the host unit that drives them
   (fdgpu_secp256k1s.cpp).  Not part of the public C ABI (that is
   include/fd_secp256k1_gpu.h). */
#pragma once

#include "../../include/fd_secp256k1_gpu.h"
#include "fdgpu_internal.h"

#ifdef __cplusplus
extern "C" {
#endif

/* All asynchronous on `stream`.

   Ingest: fdgpu_launch_precompile_ingest's contract (fdgpu_precompile.h) with
   fdt_secp256k1_walk_core as the walk: transaction i of d_txns, one per lane
   and one wave per block, is parsed into d_txn_out + 852 i, walked once to
   count the records that resolve (a count above sig_cap is
   FDGPU_CODE_PRECOMPILE_CAP and counts as none), claims its slots through the
   wave's scan and one atomic add on *d_n_rec (zero at the start), and is
   walked again to write d_descs[slot] = {msg_off, msg_sz, sig_off, addr_off}
   (arena offsets) and d_pos[slot] = instr_idx << 16 | rec_idx.  flags:
   FDGPU_SECP256K1_*. */
hipError_t fdgpu_launch_secp256k1_ingest(const uint8_t *d_arena, const fdgpu_precompile_t *d_txns, uint32_t n,
                                         uint32_t flags, uint8_t *d_txn_out, fdgpu_sig_desc_t *d_descs, uint32_t *d_pos,
                                         fdgpu_precompile_walk_t *d_walk, uint32_t *d_n_rec, hipStream_t stream);
/* Recover: one record per lane, min(*d_n_rec, cap) of them (the count stays
   on the device; cap bounds the grid): d_codes[k] = fdt_secp256k1_record_core
   of descriptor k -- 0 or FDGPU_SECP256K1_ERR_*. */
hipError_t fdgpu_launch_secp256k1_recover(const uint8_t *d_arena, const fdgpu_sig_desc_t *d_descs, uint32_t cap,
                                          const uint32_t *d_n_rec, int8_t *d_codes, hipStream_t stream);
/* Finish: fdt_secp256k1_verdict_core over transaction i's record codes
   (d_rec_codes NULL: all 0, the structural outcome alone): d_codes[i] and
   d_info + 16 i (16-B aligned). */
hipError_t fdgpu_launch_secp256k1_finish(const fdgpu_precompile_walk_t *d_walk, uint32_t n, const int8_t *d_rec_codes,
                                         const uint32_t *d_pos, int8_t *d_codes, uint8_t *d_info, hipStream_t stream);

/* Test kernels, one item per lane.
   keccak: message i = d_arena[d_off_sz[2 i], + d_off_sz[2 i + 1]) (the size
   clamped to what FDT_SECP256K1_MSG_BLOCKS blocks hold) to d_out + 32 i.
   recover: d_in + 97 i = hash | r | s | recid (d_in has 16 readable bytes
   past its end) to d_codes[i] and d_keys + 64 i.
   ops: FDGPU_SECP256K1_OPS_IN words in, FDGPU_SECP256K1_OPS_OUT out per item;
   the layouts are at fdgpu_debug_secp256k1_ops. */
hipError_t fdgpu_launch_test_keccak256(const uint8_t *d_arena, const uint32_t *d_off_sz, uint32_t n, uint32_t *d_out,
                                       hipStream_t stream);
hipError_t fdgpu_launch_test_secp256k1_recover(const uint8_t *d_in, uint32_t n, int8_t *d_codes, uint32_t *d_keys,
                                               hipStream_t stream);
hipError_t fdgpu_launch_test_secp256k1_ops(const uint32_t *d_in, uint32_t *d_out, uint32_t n, hipStream_t stream);

#define FDGPU_SECP256K1_OPS_IN  49u
#define FDGPU_SECP256K1_OPS_OUT 17u

/* The arithmetic's diagnostic, exported for tests/test_gpu_secp256k1.py
   beside the fdgpu_debug_* of include/fd_secp256k1_gpu.h (synchronous, 0 on
   success).  Item i: in[49 i ...] = op, a[8], b[8], c[8], d[8], e[8], f[8]
   (256-bit values as 8 words, least significant first; any value, also above
   the modulus, unless said otherwise), out[17 i ...] = flag, x[8], y[8]:
     0  x = a b mod p                    1  x = a^2 mod p
     2  x = 1 / a mod p (0 for 0)        3  x = a^((p+1)/4) mod p, flag = x^2 == a mod p
     4  x = a b mod n                    5  x = 1 / a mod n (0 for 0), a < n
     6  x = a mod n
     7  (x, y) = P + Q through the addition, P = (a c^2 : b c^3 : c) and Q =
        (d f^2 : e f^3 : f) with a, b, d, e < p -- the affine point (a, b)
        under the Jacobian scaling c; c = 0: infinity --; flag = 1 if the sum
        is infinity (then x = y = 0)
     8  (x, y) = 2 P through the doubling, flag as for 7 */
int fdgpu_debug_secp256k1_ops(fdgpu_engine_t *e, uint32_t const *in, uint64_t n, uint32_t *out);

#ifdef __cplusplus
}
#endif
