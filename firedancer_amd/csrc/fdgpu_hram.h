/* fdgpu_hram.h -- a signature's scalar k = SHA-512(R || A || M) mod L on the
   device, with the 32-byte field load and the wave maximum (of the lanes'
   SHA-512 block counts) its callers feed it: the verify kernels
   (fdgpu_verify.hip) and the per-stage diagnostics (fdgpu_test_kernels.hip). */
#pragma once

#include "fdgpu_internal.h"
#include "fdgpu_sc.h"
#include "fdgpu_sha512.h"

namespace fdgpu {

FDG_DEV void load32(uint32_t (&w)[8], const uint8_t *p) {
  /* 32-byte field (any 4-byte alignment in practice; use dword loads) */
  const uint32_t *q = (const uint32_t *)p;
  if (((uintptr_t)p & 3u) == 0) {
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = q[i];
  } else {
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = load_u32_unaligned(p + 4 * i);
  }
}

FDG_DEV uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, off));
  return v;
}

/* k = SHA-512(R || A || M) mod L; nb: the wave's largest block count */
FDG_DEV void hram_k(uint32_t (&k)[8], const uint32_t (&Renc)[8], const uint32_t (&Aenc)[8], const uint8_t *arena,
                    const fdgpu_sig_desc_t &d, uint32_t nb) {
  uint64_t h[8];
  sha512_hram(h, Renc, Aenc, arena + d.msg_off, d.msg_sz, nb);
  uint32_t kx[16];
#pragma unroll
  for (int j = 0; j < 8; j++) { kx[2 * j] = bswap32((uint32_t)(h[j] >> 32)); kx[2 * j + 1] = bswap32((uint32_t)h[j]); }
  sc_reduce512(k, kx);
}

}  // namespace fdgpu
