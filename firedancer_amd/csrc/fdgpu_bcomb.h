/* fdgpu_bcomb.h -- layout of the fixed-base comb tables (sizes:
   fdgpu_internal.h), shared by their build (fdgpu_bcomb.hip) and the verify
   kernels' [S]B (fdgpu_verify.hip, comb_sb):
   table i, entry j = j * 2^(W i) B as affine niels (y+x, y-x, 2dxy),
   canonical limbs, word offset ((i * ENTRIES) + j) * STRIDE. */
#pragma once

#include "fdgpu_fe.h"
#include "fdgpu_internal.h"

namespace fdgpu {

constexpr uint32_t BC_W = FDGPU_BCOMB_BITS, BC_NDIG = FDGPU_BCOMB_NDIG, BC_ENT = FDGPU_BCOMB_ENTRIES;

FDG_DEV void niels_store(uint32_t *dst, const fe &ypx, const fe &ymx, const fe &xy2d) {
#pragma unroll
  for (int i = 0; i < 10; i++) { dst[i] = ypx.v[i]; dst[10 + i] = ymx.v[i]; dst[20 + i] = xy2d.v[i]; }
  dst[30] = 0; dst[31] = 0;
}

}  // namespace fdgpu
